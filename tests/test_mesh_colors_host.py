"""CPU side of the vertex colours: the ply / obj writers and readers of python/mesh_to_sdf.py with colours, the two new entry points in
the header and the ctypes table, and the argument checks of dsdf_volume_sample that come before any device work.  (The coloured image
oracle of tests/mesh_color_cases.py is pinned against the existing volume oracle here too: the affine identity the GPU test uses.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import mesh_color_cases as MC
import mesh_oracle as M
import mesh_render_oracle as R
import sdf_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def mesh_with_colors():
    v, f = M.icosphere(0.3, 1)
    rng = np.random.default_rng(5)
    n = v / np.linalg.norm(v, axis=1, keepdims=True)
    c = rng.uniform(-0.2, 1.2, v.shape).astype(np.float32)                    # also outside [0, 1]: uchar clips, float keeps
    return v.astype(np.float32), f, n.astype(np.float32), c


@pytest.mark.parametrize('with_normals', [True, False])
def test_ply_round_trip_with_colors(tmp_path, built, with_normals):
    import mesh_to_sdf
    v, f, n, c = mesh_with_colors()
    nn = n if with_normals else None
    fn = str(tmp_path / 'u.ply')
    mesh_to_sdf.save_ply(fn, v, f, nn, colors=c)                               # uchar is the default
    head = open(fn, 'rb').read().split(b'end_header')[0].decode()
    props = re.findall(r'property (\w+) (\w+)\n', head)
    assert props == [('float', k) for k in ('x', 'y', 'z') + (('nx', 'ny', 'nz') if with_normals else ())] + \
        [('uchar', k) for k in ('red', 'green', 'blue')]
    v2, f2, c2 = mesh_to_sdf.load_mesh_indexed(fn, colors=True)
    assert np.array_equal(v2, v) and np.array_equal(f2, f) and c2.dtype == np.float32 and c2.shape == v.shape
    k = np.rint(np.clip(c.astype(np.float64), 0, 1) * 255)
    assert np.array_equal(np.rint(c2.astype(np.float64) * 255), k) and np.abs(c2 - k / 255).max() < 1e-7
    assert np.abs(c2 - np.clip(c, 0, 1)).max() <= 0.5 / 255 + 1e-7
    fn = str(tmp_path / 'f.ply')
    mesh_to_sdf.save_ply(fn, torch.from_numpy(v), torch.from_numpy(f.astype(np.int32)), nn, colors=torch.from_numpy(c), color_dtype='float')
    v2, f2, c2 = mesh_to_sdf.load_mesh_indexed(fn, colors=True)
    assert np.array_equal(v2, v) and np.array_equal(f2, f) and np.array_equal(c2, c)      # lossless, unclipped
    # the two-tuple readers return what they returned
    for got in (mesh_to_sdf.load_mesh_indexed(fn), mesh_to_sdf.load_ply(fn)):
        assert len(got) == 2 and np.array_equal(got[0], v) and np.array_equal(got[1], f)
    assert np.array_equal(mesh_to_sdf.load_mesh(fn), v[f])
    # without colours: the file of before, and None for the colours
    fn = str(tmp_path / 'n.ply')
    mesh_to_sdf.save_ply(fn, v, f, nn)
    assert b'red' not in open(fn, 'rb').read().split(b'end_header')[0]
    v2, f2, c2 = mesh_to_sdf.load_mesh_indexed(fn, colors=True)
    assert np.array_equal(v2, v) and np.array_equal(f2, f) and c2 is None
    assert os.path.getsize(fn) == len(open(fn, 'rb').read().split(b'end_header\n')[0]) + 11 + len(v) * (24 if with_normals else 12) + len(f) * 13


def test_ascii_ply_written_by_hand(tmp_path, built):
    import mesh_to_sdf
    (tmp_path / 'a.ply').write_text('ply\nformat ascii 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\n'
                                    'property uchar red\nproperty uchar green\nproperty uchar blue\nproperty uchar alpha\n'
                                    'element face 2\nproperty list uchar int vertex_indices\nend_header\n'
                                    '0 0 0 255 0 0 255\n1 0 0 0 128 0 255\n1 1 0 0 0 51 255\n0 1 0 255 255 255 0\n3 0 1 2\n3 0 2 3\n')
    v, f, c = mesh_to_sdf.load_mesh_indexed(str(tmp_path / 'a.ply'), colors=True)
    assert v.shape == (4, 3) and f.tolist() == [[0, 1, 2], [0, 2, 3]]
    np.testing.assert_allclose(c, np.array([[1, 0, 0], [0, 128 / 255, 0], [0, 0, 0.2], [1, 1, 1]]), rtol=0, atol=1e-7)
    assert c.dtype == np.float32
    # a file with only some of the three channels has no colours
    (tmp_path / 'r.ply').write_text('ply\nformat ascii 1.0\nelement vertex 3\nproperty float x\nproperty float y\nproperty float z\n'
                                    'property uchar red\nelement face 1\nproperty list uchar int vertex_indices\nend_header\n'
                                    '0 0 0 9\n1 0 0 9\n1 1 0 9\n3 0 1 2\n')
    assert mesh_to_sdf.load_mesh_indexed(str(tmp_path / 'r.ply'), colors=True)[2] is None


def test_obj_round_trip_with_colors(tmp_path, built):
    import mesh_to_sdf
    v, f, n, c = mesh_with_colors()
    for nn in (n, None):
        fn = str(tmp_path / 'c.obj')
        mesh_to_sdf.save_obj(fn, v, f, nn, colors=c)
        first = open(fn).readline().split()
        assert first[0] == 'v' and len(first) == 7
        v2, f2, c2 = mesh_to_sdf.load_mesh_indexed(fn, colors=True)
        assert np.array_equal(v2, v) and np.array_equal(f2, f) and np.array_equal(c2, c)  # %.9g: float32 round-trips
        for got in (mesh_to_sdf.load_mesh_indexed(fn), mesh_to_sdf.load_obj(fn)):
            assert len(got) == 2 and np.array_equal(got[0], v) and np.array_equal(got[1], f)
        fn = str(tmp_path / 'p.obj')
        mesh_to_sdf.save_obj(fn, v, f, nn)
        assert len(open(fn).readline().split()) == 4
        assert mesh_to_sdf.load_mesh_indexed(fn, colors=True)[2] is None
    M.write_obj(str(tmp_path / 'o.obj'), v, f)
    assert mesh_to_sdf.load_obj(str(tmp_path / 'o.obj'), colors=True)[2] is None


def test_wrong_color_shape_raises(tmp_path, built):
    import mesh_to_sdf
    v, f, n, c = mesh_with_colors()
    for save in (mesh_to_sdf.save_ply, mesh_to_sdf.save_obj):
        for bad in (c[:-1], c[:, :2], np.concatenate([c, c[:, :1]], 1), c.reshape(-1)):
            with pytest.raises(ValueError, match='colors'):
                save(str(tmp_path / ('x.ply' if save is mesh_to_sdf.save_ply else 'x.obj')), v, f, n, colors=bad)
    with pytest.raises(ValueError, match='color_dtype'):
        mesh_to_sdf.save_ply(str(tmp_path / 'x.ply'), v, f, n, colors=c, color_dtype='double')
    assert 'no gamma' in mesh_to_sdf.save_ply.__doc__ and 'linear' in mesh_to_sdf.save_ply.__doc__.lower()


def test_scene_mesh_loader_returns_corner_colors(tmp_path, built, monkeypatch):
    import mesh_to_sdf
    import scenes
    v, f, n, c = mesh_with_colors()
    for name, cols in (('tinted', np.clip(c, 0, 1)), ('bare', None)):
        d = tmp_path / 'scenes' / name
        d.mkdir(parents=True)
        mesh_to_sdf.save_ply(str(d / f'{name}.ply'), v, f, colors=cols, color_dtype='float')
    monkeypatch.setattr(scenes, 'SCENE_DIR', str(tmp_path / 'scenes'))
    tri, nrm, cc = scenes.load_target_mesh('tinted', device='cpu', colors=True)
    assert tuple(cc.shape) == tuple(tri.shape) == (len(f), 3, 3) and cc.dtype == torch.float32 and cc.is_contiguous()
    assert np.array_equal(cc.numpy(), np.clip(c, 0, 1)[f]) and np.array_equal(tri.numpy(), v[f] + np.float32(0.5))
    assert len(scenes.load_target_mesh('tinted', device='cpu')) == 2
    assert scenes.load_target_mesh('bare', device='cpu', colors=True)[2] is None
    assert scenes.load_target_mesh('absent', colors=True) is None


def test_new_symbols_declared_and_bound(built):
    import dsdf
    txt = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'dsdf.h')).read(), flags=re.S)
    lib = dsdf.load()
    for name, nargs in (('dsdf_volume_sample', 9), ('dsdf_mesh_render_forward_colors', 16)):
        m = re.search(r'\bint\s+' + name + r'\s*\(([^;]*)\)\s*;', txt)
        assert m, f'{name} is not declared in include/dsdf.h'
        assert len(m.group(1).split(',')) == nargs == len(dsdf._lib.SYMBOLS[name][1])
        assert hasattr(lib, name)
    # the coloured entry is the plain one with one more pointer behind the buffer
    assert dsdf._lib.SYMBOLS['dsdf_mesh_render_forward_colors'][1][2:] == dsdf._lib.SYMBOLS['dsdf_mesh_render_forward'][1][1:]
    xf = os.path.join(ROOT, 'differentiable-sdf-rendering_amd', 'lib', 'variants', 'libdsdf_xf.so')
    if os.path.isfile(xf):                                                     # the other build of the library exports them too
        other = C.CDLL(xf)
        assert hasattr(other, 'dsdf_volume_sample') and hasattr(other, 'dsdf_mesh_render_forward_colors')
    assert lib.dsdf_version() == 308
    assert 'sample_volume' in dir(dsdf)


def test_volume_sample_refuses_bad_arguments_before_device_work(built):
    import dsdf
    lib = dsdf.load()
    one = C.c_void_p(16)                                                      # never dereferenced: validation fails first
    for args in ((one, 4, 4, 4, 2, one, 8, one), (one, 4, 4, 4, 0, one, 8, one), (one, 0, 4, 4, 3, one, 8, one), (one, 4, 4, -2, 1, one, 8, one),
                 (None, 4, 4, 4, 3, one, 8, one), (one, 4, 4, 4, 3, None, 8, one), (one, 4, 4, 4, 3, one, 8, None), (one, 4, 4, 4, 3, one, -1, one)):
        assert lib.dsdf_volume_sample(*args, None) == -1 and b'dsdf_volume_sample:' in lib.dsdf_last_error(), args
    assert b'channels' in (lib.dsdf_volume_sample(one, 4, 4, 4, 2, one, 8, one, None), lib.dsdf_last_error())[1]
    assert lib.dsdf_volume_sample(one, 4, 4, 4, 3, one, 0, one, None) == 0    # n = 0: no launch
    # the coloured render: the checks of dsdf_mesh_render_forward, and a shading without a volume is fine only with colours
    p = dsdf.default_params()
    cam = (dsdf.DsdfCamera * 1)()
    seeds = (C.c_uint32 * 1)(1)
    sh = dsdf.DsdfShading()
    call = lambda colors, shading, ws=16: lib.dsdf_mesh_render_forward_colors(one, colors, C.byref(p), cam, 1, 16, 16, 4, None, seeds, 2, shading,
                                                                              one, one, ws, None)
    assert call(None, C.byref(sh)) == -1 and b'dsdf_shading' in lib.dsdf_last_error()
    assert call(one, None) == -1 and b'dsdf_shading' in lib.dsdf_last_error()
    assert call(one, C.byref(sh)) == -2 and b'workspace too small' in lib.dsdf_last_error()      # past the shading check
    sh.use_mis = 1
    assert call(one, C.byref(sh)) == -1 and b'use_mis' in lib.dsdf_last_error()


def test_shading_without_albedo_is_refused_by_to_struct(built):
    import dsdf
    with pytest.raises(dsdf.DsdfError, match='corner colours'):
        dsdf.Shading(None, 0.8).to_struct(1, 16)
    st, keep = dsdf.Shading(None, 0.8, hide_emitters=True).to_struct(1, 16, need_albedo=False)
    assert not st.albedo and st.hide_emitters == 1 and abs(st.env_radiance[1] - 0.8) < 1e-7 and keep == []


def test_colored_oracle_equals_volume_oracle_on_an_affine_field():
    """The identity behind the GPU test: barycentric interpolation of c = A p + b at the corners IS the trilinear lookup of the volume
    that holds c at its texel centres (inside [0.5 / res, 1 - 0.5 / res]^3), so the two fp64 references agree to rounding."""
    v, f = M.icosphere(0.3, 1, centre=(0.05, -0.02, 0.01))
    tri = (v + np.float32(0.5))[f].astype(np.float64)
    cam = O.Camera(O.regular_camera_origins(3)[1]).rounded()
    W = H = 8
    spp = 4
    g = torch.Generator().manual_seed(1)
    n = (W + 4) * (H + 4) * spp
    offsets, emitter = torch.rand(n, 2, generator=g), torch.rand(n, 2, generator=g)
    vol = torch.from_numpy((MC.texel_centres() @ MC.AFFINE_A.T + MC.AFFINE_B).reshape(*MC.VOLUME_SHAPE, 3))     # fp64, unrounded
    prim = R.primary(tri, cam, W, H, spp, offsets)
    a = R.render(tri, None, cam, W, H, spp, offsets, O.DIRECT, albedo=vol, emitter_u=emitter, env=0.8, prim=prim)
    b = MC.render_colors(tri, None, tri @ MC.AFFINE_A.T + MC.AFFINE_B, cam, W, H, spp, offsets, emitter, env=0.8, prim=prim)
    assert a.max() > 0.1 and np.abs(a - 0.8).max() > 0.1                       # the mesh is in view
    assert np.abs(a - b).max() < 1e-13
    pts = MC.sample_points()
    assert pts.shape[0] == 1000 + 5 * 6 * 7 + 8 * (5 + 6 + 7) and float(pts.min()) < 0 and float(pts.max()) > 1
