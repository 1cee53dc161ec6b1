"""GPU tests of the vertex colours: dsdf.sample_volume (dsdf_volume_sample) against the fp64 trilinear lookup of the oracle; the mesh
render with a reflectance per triangle corner (dsdf.MeshBvh(colors=), dsdf_mesh_render_forward_colors) against the existing volume
reference through an affine colour field and against the coloured oracle of tests/mesh_color_cases.py; the colours dsdf.extract_mesh
bakes, through both renderers and through the command line.  Film, cameras, samples, meshes and the gate are those of
tests/test_gpu_mesh_render.py."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import iso_cases as I
import mesh_color_cases as MC
import mesh_render_oracle as R
import precision as P
import sdf_oracle as O
import test_gpu_mesh_render as T

pytestmark = pytest.mark.gpu

ENV = T.ENV
RT_W = RT_H = 24                             # the round trip: film and samples of tests/test_gpu_iso.py
RT_SPP = 8


@pytest.fixture(scope='module')
def dsdf(built):
    import dsdf as m
    m.load()
    assert torch.cuda.is_available()
    return m


# ---- 1. sample_volume ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def random_volume(channels):
    return torch.rand(*MC.VOLUME_SHAPE, channels, generator=torch.Generator().manual_seed(10 + channels))


@pytest.mark.parametrize('channels', [3, 1])
def test_sample_volume_matches_fp64_lookup(dsdf, channels):
    """Max abs error <= 1e-6 against O.eval_trilinear in fp64 of the same fp32 inputs: values of O(1), an 8-tap fp32 sum."""
    vol = random_volume(channels)
    pts = MC.sample_points()
    ref = O.eval_trilinear(vol.double(), pts.double()).numpy()
    volg, ptsg = vol.cuda(), pts.cuda()
    for n in (pts.shape[0], 257, 1, 0):
        got = dsdf.sample_volume(volg, ptsg[:n])
        assert tuple(got.shape) == (n, channels) and got.dtype == torch.float32 and got.is_cuda
        err = float(np.abs(got.cpu().numpy() - ref[:n]).max()) if n else 0.0
        print(f'sample_volume C={channels} n={n}: max abs error {err:.3e}')
        assert err <= 1e-6, (channels, n, err)
    if channels == 1:                                                         # (Z,Y,X) is (Z,Y,X,1)
        assert torch.equal(dsdf.sample_volume(volg[..., 0], ptsg), dsdf.sample_volume(volg, ptsg))
    # the single points are the LAST ones too (a cell-face point), not only a random one
    assert torch.equal(dsdf.sample_volume(volg, ptsg[-1:]), dsdf.sample_volume(volg, ptsg)[-1:])


def test_sample_volume_argument_validation(dsdf):
    lib = dsdf.load()
    vol = torch.zeros(2, 3, 4, 3, device='cuda'); pts = torch.zeros(5, 3, device='cuda'); out = torch.zeros(5, 3, device='cuda')
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None

    def call(volume=vol, dims=(4, 3, 2), channels=3, points=pts, n=5, o=out):
        return lib.dsdf_volume_sample(p(volume), *dims, channels, p(points), n, p(o), None)
    for kwargs in (dict(volume=None), dict(points=None), dict(o=None), dict(channels=2), dict(channels=0), dict(channels=4),
                   dict(dims=(0, 3, 2)), dict(dims=(4, 0, 2)), dict(dims=(4, 3, -1)), dict(n=-1)):
        assert call(**kwargs) == -1 and b'dsdf_volume_sample:' in lib.dsdf_last_error(), kwargs
    assert call(n=0, points=None, o=None) == 0                                # nothing to do: no launch, no pointer needed
    assert call() == 0
    with pytest.raises(dsdf.DsdfError, match='C = 1 or 3'):
        dsdf.sample_volume(torch.zeros(2, 2, 2, 2, device='cuda'), pts)
    with pytest.raises(dsdf.DsdfError, match=r'\(N,3\)'):
        dsdf.sample_volume(vol, torch.zeros(5, 2, device='cuda'))
    with pytest.raises(dsdf.DsdfError, match='no CPU path'):
        dsdf.sample_volume(vol.cpu(), pts)


# ---- the mesh render with corner colours -------------------------------------------------------------------------------------------
def normals_of(name, smooth):
    tri, ns, nf = T.mesh(name)
    return ns if smooth else (None if smooth is None else nf)


def gpu_render_colors(dsdf, name, spp, smooth, colors, hide=False, views=None, albedo=None):
    tri = T.mesh(name)[0]
    nrm = normals_of(name, smooth)
    bvh = dsdf.MeshBvh(torch.from_numpy(tri).cuda(), None if nrm is None else torch.from_numpy(nrm).cuda(),
                       colors=None if colors is None else torch.from_numpy(colors).cuda())
    sens, _ = T.cameras(dsdf)
    offsets, emitter = T.samples(spp)
    vs = list(range(T.NV)) if views is None else views
    return dsdf.mesh_render(bvh, [sens[v] for v in vs], spp, offsets=offsets[vs].cuda(), integrator='sdf_direct_reparam',
                            shading=dsdf.Shading(albedo, ENV, hide_emitters=hide), emitter_samples=emitter[vs].cuda()).cpu().numpy()


@functools.lru_cache(maxsize=None)
def affine_reference(name, spp):
    """The EXISTING reference, R.render over a reflectance volume, with the affine volume."""
    import dsdf
    tri, ns, _ = T.mesh(name)
    _, cams = T.cameras(dsdf)
    offsets, emitter = T.samples(spp)
    prim = T.primaries(name, spp)
    return np.stack([R.render(tri, ns, cams[v], T.W, T.H, spp, offsets[v], O.DIRECT, albedo=MC.affine_volume(), emitter_u=emitter[v], env=ENV,
                              prim=prim[v]) for v in range(T.NV)])


@pytest.mark.parametrize('spp', [64, 4])
@pytest.mark.parametrize('name', ['sphere', 'box', 'two_spheres'])
def test_affine_colors_equal_the_volume_reference(dsdf, name, spp):
    """2. A volume holding c = A p + b at its texel centres is that function inside [0.5 / res, 1 - 0.5 / res]^3, and so is the
    barycentric interpolation of c(corner): the coloured render must pass the gate against the reference that reads the volume."""
    tri = T.mesh(name)[0]
    lo = 0.5 / min(MC.VOLUME_SHAPE)
    assert tri.min() >= lo and tri.max() <= 1 - lo                            # the mesh lies in the exact region of the volume
    img = gpu_render_colors(dsdf, name, spp, True, MC.affine_colors(tri))
    T.check(img, affine_reference(name, spp), spp, f'affine colours {name}/spp{spp}')


@functools.lru_cache(maxsize=None)
def random_colors(name):
    n = T.mesh(name)[0].shape[0]
    return torch.rand(n, 3, 3, generator=torch.Generator().manual_seed(3)).numpy()


@functools.lru_cache(maxsize=None)
def colored_reference(name, spp, smooth, hide=False):
    import dsdf
    tri = T.mesh(name)[0]
    _, cams = T.cameras(dsdf)
    offsets, emitter = T.samples(spp)
    prim = T.primaries(name, spp)
    return np.stack([MC.render_colors(tri, normals_of(name, smooth), random_colors(name), cams[v], T.W, T.H, spp, offsets[v], emitter[v],
                                      env=ENV, hide_emitters=hide, prim=prim[v]) for v in range(T.NV)])


@pytest.mark.parametrize('spp', [64, 4])
@pytest.mark.parametrize('smooth', [True, None], ids=['stored-normals', 'no-normals'])
def test_random_corner_colors_match_oracle(dsdf, smooth, spp):
    """3. Colours that jump across every edge: a permuted corner, or a lookup by slot instead of by original index, is another image."""
    tri = T.mesh('sphere')[0]
    assert tri.shape[0] > 4
    order = dsdf.MeshBvh(torch.from_numpy(tri).cuda()).order.cpu().numpy()
    assert not np.array_equal(order, np.arange(len(order)))                   # the Morton order is not the caller's order
    cols = random_colors('sphere')
    ref = colored_reference('sphere', spp, smooth)
    T.check(gpu_render_colors(dsdf, 'sphere', spp, smooth, cols), ref, spp, f'random colours smooth={smooth}/spp{spp}')
    if spp == 64 and smooth:                                                  # the reference does tell the mistakes apart
        for wrong in (cols[:, [1, 2, 0]], cols[order]):
            bad = np.stack([MC.render_colors(tri, normals_of('sphere', smooth), wrong, T.cameras(dsdf)[1][0], T.W, T.H, spp, T.samples(spp)[0][0],
                                             T.samples(spp)[1][0], env=ENV, prim=T.primaries('sphere', spp)[0])])
            assert P.rel_l2(bad[0], ref[0]) > 100 * T.FWD_TOL


def test_batch_fallback_occlusion_and_hidden_emitters(dsdf):
    """4. Views of one call equal single-view calls; without colours the call is dsdf_mesh_render_forward; the other integrators ignore
    the colours; hide_emitters and the shadow query act on a coloured mesh."""
    cols = random_colors('sphere')
    img = gpu_render_colors(dsdf, 'sphere', 64, True, cols)
    for v in range(T.NV):
        assert P.rel_l2(gpu_render_colors(dsdf, 'sphere', 64, True, cols, views=[v])[0], img[v]) < 1e-6
    # colors=None: dsdf_mesh_render_forward itself.  (The film is summed with float atomics in no fixed order, so two calls of the SAME
    # entry point differ in the last bits: "the same render" is measured the way tests/test_gpu_mesh_render.py measures it.)
    tri, ns, _ = T.mesh('sphere')
    trig, nsg = torch.from_numpy(tri).cuda(), torch.from_numpy(ns).cuda()
    plain = dsdf.MeshBvh(trig, nsg)
    assert plain.colors is None
    sens, _ = T.cameras(dsdf)
    offsets, emitter = T.samples(4)
    sh = dsdf.Shading(T.albedo_volume().cuda(), ENV)
    a = dsdf.mesh_render(plain, sens, 4, offsets=offsets.cuda(), integrator='sdf_direct_reparam', shading=sh, emitter_samples=emitter.cuda())
    lib = dsdf.load()
    st, keep = sh.to_struct(T.NV, (T.W + 4) * (T.H + 4) * 4, emitter.cuda())
    cams = (dsdf.DsdfCamera * T.NV)(*[s.to_struct() for s in sens])
    b = torch.empty_like(a)
    ws = torch.empty(int(lib.dsdf_mesh_render_workspace_size(T.W, T.H, T.NV)), dtype=torch.uint8, device='cuda')
    offg = offsets.cuda().contiguous()
    prm = dsdf.default_params()
    rc = lib.dsdf_mesh_render_forward(C.c_void_p(plain.buffer.data_ptr()), C.byref(prm), cams, T.NV, T.W, T.H, 4, C.c_void_p(offg.data_ptr()), None,
                                      dsdf.DSDF_DIRECT, C.byref(st), C.c_void_p(b.data_ptr()), C.c_void_p(ws.data_ptr()), ws.numel(),
                                      C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.dsdf_last_error()
    assert P.rel_l2(a.cpu().numpy(), b.cpu().numpy()) < 1e-6
    T.check(a.cpu().numpy(), T.reference('sphere', 4, 'direct', True), 4, 'no colours: the volume render')
    colored = dsdf.MeshBvh(trig, nsg, colors=torch.from_numpy(cols).cuda())
    assert colored.colors.is_contiguous() and tuple(colored.colors.shape) == (tri.shape[0], 3, 3) and torch.equal(colored.buffer.view(torch.int32), plain.buffer.view(torch.int32))        # (the layout does not change)
    for integ in (dsdf.DSDF_SILHOUETTE, dsdf.DSDF_SIMPLE_SHADING):
        assert P.rel_l2(dsdf.mesh_render(colored, sens, 4, offsets=offg, integrator=integ).cpu().numpy(),
                        dsdf.mesh_render(plain, sens, 4, offsets=offg, integrator=integ).cpu().numpy()) < 1e-6
    # a Shading without a volume serves a coloured mesh only
    with pytest.raises(dsdf.DsdfError, match='corner colours'):
        dsdf.mesh_render(plain, sens, 4, offsets=offg, integrator='sdf_direct_reparam', shading=dsdf.Shading(None, ENV))
    grid = dsdf.SdfGrid(torch.from_numpy(I.grid('sphere16')).float().cuda())
    with pytest.raises(dsdf.DsdfError, match='corner colours'):
        dsdf.render_forward(grid, sens, 4, offsets=offg, integrator='sdf_direct_reparam', shading=dsdf.Shading(None, ENV))
    with pytest.raises(dsdf.DsdfError, match=r'\(T,3,3\)'):
        dsdf.MeshBvh(trig, nsg, colors=torch.zeros(tri.shape[0], 3, device='cuda'))
    # occlusion and hidden emitters, on the two spheres that shadow each other
    cols2 = random_colors('two_spheres')
    both = colored_reference('two_spheres', 64, True)
    hid = colored_reference('two_spheres', 64, True, True)
    T.check(gpu_render_colors(dsdf, 'two_spheres', 64, True, cols2), both, 64, 'two_spheres/colours')
    T.check(gpu_render_colors(dsdf, 'two_spheres', 64, True, cols2, hide=True), hid, 64, 'two_spheres/colours/hidden')
    assert np.abs(both[:, 0, 0] - ENV).max() < 1e-12 and np.abs(hid[:, 0, 0]).max() == 0.0
    # (that the reference of this mesh has shadows in it is asserted by tests/test_gpu_mesh_render.py: the shadow query is shared)


# ---- the colours extract_mesh bakes -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def round_trip_view():
    import dsdf
    sensor = dsdf.get_regular_cameras(3, resx=RT_W, resy=RT_H)[1]
    cam = O.Camera.from_params(np.frombuffer(bytes(sensor.to_struct()), np.float32, 16))
    g = torch.Generator().manual_seed(7)
    n = (RT_W + 4) * (RT_H + 4) * RT_SPP
    offsets = torch.rand(n, 2, generator=g)
    emitter = torch.rand(n, 2, generator=g)
    return sensor, cam, offsets, emitter


def oracle_distance(n):
    """d(n) of the fp64 reference: the oracle's mesh with O.eval_trilinear colours at its vertices, rendered by the coloured mesh oracle,
    against O.render of the SDF with the volume; mean absolute difference."""
    _, cam, offsets, emitter = round_trip_view()
    alb = T.albedo_volume().double()
    m = I.oracle_mesh_of('sphere16', (n, n, n))
    cv = O.eval_trilinear(alb, torch.from_numpy(m['positions'])).numpy()
    f = m['faces']
    mesh_img = MC.render_colors(m['positions'][f], m['normals'][f], cv[f], cam, RT_W, RT_H, RT_SPP, offsets, emitter, env=ENV)
    sdf = O.Grid3d(torch.from_numpy(I.grid('sphere16')))
    sdf_img = O.render(sdf, cam, RT_W, RT_H, RT_SPP, offsets.double(), integrator=O.DIRECT, reparam=False, albedo=alb,
                       emitter_u=emitter.double(), env=ENV).detach().numpy()
    return float(np.abs(mesh_img - sdf_img).mean())


def gpu_distances(dsdf, grid, n):
    """(d(n), d_grey(n)): the coloured extracted mesh, and the same mesh with every vertex at the mean colour, against the SDF render."""
    sensor, _, offsets, emitter = round_trip_view()
    alb = T.albedo_volume().cuda()
    v, f, nrm, col = dsdf.extract_mesh(grid, resolution=n, colors=alb)
    assert tuple(col.shape) == tuple(v.shape) and col.dtype == torch.float32
    off, emi = offsets[None].cuda(), emitter[None].cuda()
    sdf_img = dsdf.render_forward(grid, [sensor], RT_SPP, offsets=off, integrator=dsdf.DSDF_DIRECT, reparam=False,
                                  shading=dsdf.Shading(alb, ENV), emitter_samples=emi)
    assert float((sdf_img - ENV).abs().mean()) > 0.01                         # the object is in the picture
    out = []
    for c in (col, col.mean(0, keepdim=True).expand_as(col).contiguous()):
        bvh = dsdf.MeshBvh(v[f.long()], nrm[f.long()], colors=c[f.long()])
        img = dsdf.mesh_render(bvh, [sensor], RT_SPP, offsets=off, integrator=dsdf.DSDF_DIRECT, shading=dsdf.Shading(None, ENV),
                               emitter_samples=emi)
        out.append(float((img - sdf_img).abs().mean()))
    return out


def test_round_trip_through_both_renderers(dsdf):
    """5. mesh_render(extract_mesh(sdf, colors=albedo)) against render_forward(sdf, Shading(albedo)): at n = 32 the GPU must not be further
    from its SDF render than the fp64 reference is at n = 16, and a mesh that ignores the colours (every vertex grey) must be five times
    that far.  fp64 reference with these samples: d(8) = 3.1e-3, d(16) = 8.3e-4, d(32) = 4.2e-5; grey d(32) = 5.9e-3.  Measured on the
    MI355X: d(32) = 4.25e-5, d(16) = 8.31e-4, grey d(32) = 5.94e-3."""
    grid = dsdf.SdfGrid(torch.from_numpy(I.grid('sphere16')).float().cuda())
    d16_ref = oracle_distance(16)
    d32, d32_grey = gpu_distances(dsdf, grid, 32)
    d16, _ = gpu_distances(dsdf, grid, 16)
    print(f'coloured round trip: oracle d(16) = {d16_ref:.3e}, GPU d(32) = {d32:.3e}, GPU d(16) = {d16:.3e}, GPU grey d(32) = {d32_grey:.3e}')
    assert 0 < d32 <= d16_ref, (d32, d16_ref)
    assert d32_grey >= 5 * d16_ref, (d32_grey, d16_ref)


def test_colors_are_sampled_at_the_world_space_vertices(dsdf):
    """6. With sdf.p (and with a general to_world) the colours are the volume at the vertices the call RETURNS."""
    alb = T.albedo_volume().cuda()
    data = torch.from_numpy(I.grid('sphere16')).float().cuda()
    grid = dsdf.SdfGrid(data)
    v0, f0, n0, c0 = dsdf.extract_mesh(grid, resolution=16, colors=alb)
    assert torch.equal(c0, dsdf.sample_volume(alb, v0))
    plain = dsdf.extract_mesh(grid, resolution=16)
    assert len(plain) == 3 and torch.equal(plain[0], v0) and torch.equal(plain[1], f0) and torch.equal(plain[2], n0)
    v, f, c = dsdf.extract_mesh(grid, resolution=16, normals=False, colors=alb)
    assert torch.equal(v, v0) and torch.equal(c, c0)
    grid.set_translation((0.0625, -0.03125, 0.125))
    v1, f1, n1, c1 = dsdf.extract_mesh(grid, resolution=16, colors=alb)
    assert torch.equal(f1, f0) and not torch.equal(v1, v0)
    assert torch.equal(c1, dsdf.sample_volume(alb, v1))
    assert float((c1 - c0).abs().max()) > 1e-2                                # not the lookup at the untranslated vertices
    c, s = np.cos(0.4), np.sin(0.4)
    tw = np.array([[0.8 * c, -0.8 * s, 0, 0.25], [0.8 * s, 0.8 * c, 0, -0.05], [0, 0, 0.9, 0.05], [0, 0, 0, 1]])
    gt = dsdf.SdfGrid(data, to_world=tw).set_translation((0.01, 0.02, 0.03))
    v2, _, _, c2 = dsdf.extract_mesh(gt, resolution=16, colors=alb)
    assert torch.equal(c2, dsdf.sample_volume(alb, v2)) and float((c2 - c0).abs().max()) > 1e-2
    # no surface: (0, 3)
    empty = dsdf.extract_mesh(dsdf.SdfGrid(torch.full((8, 8, 8), 0.5, device='cuda')), colors=alb)
    assert len(empty) == 4 and all(tuple(t.shape) == (0, 3) for t in empty)
    with pytest.raises(dsdf.DsdfError, match=r'\(Z,Y,X,3\)'):
        dsdf.extract_mesh(grid, colors=alb[..., :1].contiguous())


@pytest.mark.parametrize('float_colors', [False, True], ids=['uchar', 'float'])
def test_extract_mesh_cli_writes_colors(dsdf, tmp_path, float_colors):
    """7. `extract_mesh.py sdf.vol --albedo albedo.vol -o out.ply`: V colours, within half a uchar step of sample_volume at the vertices
    of the file -- exactly with --float-colors -- and a mesh the --meshrefs loader takes with its colours."""
    import extract_mesh
    import mesh_to_sdf
    import util
    util.write_vol(str(tmp_path / 'sdf.vol'), torch.from_numpy(I.grid('sphere16')).float())
    util.write_vol(str(tmp_path / 'albedo.vol'), T.albedo_volume())
    out = str(tmp_path / 'out.ply')
    assert extract_mesh.main([str(tmp_path / 'sdf.vol'), '--albedo', str(tmp_path / 'albedo.vol'), '-o', out] +
                             (['--float-colors'] if float_colors else [])) == 0
    v, f, c = mesh_to_sdf.load_mesh_indexed(out, colors=True)
    assert len(v) > 100 and c is not None and c.shape == v.shape and c.dtype == np.float32
    want = dsdf.sample_volume(util.read_vol(str(tmp_path / 'albedo.vol')).float().contiguous(), torch.from_numpy(v).cuda()).cpu().numpy()
    if float_colors:
        err = float(np.abs(c - want).max())
        assert err == 0.0, err
    else:
        k = np.rint(c.astype(np.float64) * 255)                                # the stored uchar (c is its fp32 quotient by 255)
        assert np.abs(k / 255 - c).max() < 1e-7
        err = float(np.abs(k - want.astype(np.float64) * 255).max()) / 255
        assert err <= 0.5 / 255, err
    print(f'extract_mesh.py --albedo ({"float" if float_colors else "uchar"}): {len(v)} vertices, max colour error {err:.3e}')
    v2, f2 = mesh_to_sdf.load_mesh_indexed(out)
    assert np.array_equal(v2, v) and np.array_equal(f2, f)


def test_meshrefs_shade_with_the_colours_of_the_scene_mesh(dsdf, tmp_path, monkeypatch):
    """The whole loop: the ply `extract_mesh.py --albedo` writes, as a scene's mesh, gives `optimize.py --meshrefs` (sdf_direct_reparam,
    a diffuse config) reference images shaded with ITS colours, not with the procedural stand-in volume."""
    import extract_mesh
    import mesh_to_sdf
    import optimize
    import scenes
    import util
    from configs import apply_cmdline_args, get_config
    from opt_configs import get_opt_config
    util.write_vol(str(tmp_path / 'sdf.vol'), torch.from_numpy(I.grid('sphere16')).float())
    util.write_vol(str(tmp_path / 'albedo.vol'), T.albedo_volume())
    out = str(tmp_path / 'out.ply')
    assert extract_mesh.main([str(tmp_path / 'sdf.vol'), '--albedo', str(tmp_path / 'albedo.vol'), '--float-colors', '-o', out]) == 0
    v, f, c = mesh_to_sdf.load_mesh_indexed(out, colors=True)
    d = tmp_path / 'scenes' / 'tinted'
    d.mkdir(parents=True)
    mesh_to_sdf.save_ply(str(d / 'tinted.ply'), v - np.float32(0.5), f, colors=c, color_dtype='float')    # scene meshes live in [-0.5, 0.5]^3
    monkeypatch.setattr(scenes, 'SCENE_DIR', str(tmp_path / 'scenes'))
    monkeypatch.setattr(optimize, 'RENDER_DIR', str(tmp_path / 'renders'))
    config = get_config('warp')
    remaining = apply_cmdline_args(config, ['--resx=24', '--resy=24'], return_dict=True)
    oc, _ = get_opt_config('diffuse-6', remaining)
    oc.scene = 'tinted'
    assert config.integrator == 'sdf_direct_reparam'
    optimize.render_reference_images(oc, config, ref_spp=64, mesh_refs=True)
    ref0 = np.load(tmp_path / 'renders' / 'tinted' / oc.name / config.integrator / 'ref' / 'ref-00.npy')
    assert ref0.shape == (24, 24, 3)
    tri, nrm, cc = scenes.load_target_mesh('tinted', colors=True)
    assert cc is not None and tuple(cc.shape) == tuple(tri.shape)
    render = lambda bvh, sh: dsdf.mesh_render(bvh, [oc.sensors[0]], 64, seeds=[41], integrator='sdf_direct_reparam', shading=sh)[0].cpu().numpy()
    want = render(dsdf.MeshBvh(tri, nrm, colors=cc), dsdf.Shading(None, 1.0))
    standin = render(dsdf.MeshBvh(tri, nrm), dsdf.Shading(scenes.load_target_albedo('tinted'), 1.0))
    assert np.abs(want - 1.0).mean() > 0.01                                    # the mesh is in the picture
    assert P.rel_l2(ref0, want) < 1e-6 and P.rel_l2(ref0, standin) > 1e-2
    # the principled configs keep raising
    oc2, _ = get_opt_config('principled-6', apply_cmdline_args(get_config('warp'), ['--resx=24', '--resy=24'], return_dict=True))
    oc2.scene = 'tinted'
    with pytest.raises(NotImplementedError, match='principled'):
        optimize.render_reference_images(oc2, config, ref_spp=64, mesh_refs=True)
