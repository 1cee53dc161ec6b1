"""GPU checks of the mesh simplification (include/dsdf.h: dsdf_simplify_keys / _mark / _emit; dsdf.simplify_mesh and the two command
lines) against the HOST build of the same statements (tests/harness/dsdf_simplify_host.cpp) and the fp64 reference in another
formulation (tests/mesh_simplify_oracle.py).

BITS.  The arithmetic is uncontracted and uses only + - x / sqrtf, correctly rounded in both builds, and one lane sums a cell in the
order of the host's loop: faces, positions, normals and colours of the device are `==` the host build's.  A difference is a finding.
GATE.  mesh_simplify_oracle.GATE = 4 x the maximum fp32 error of the positions measured on the host build, in cell sizes
(tests/test_mesh_simplify_host.py); the device, returning the host's bits, has the host's error.
Measured on the MI355X: `==` the host build on every case, max |x_fp32 - x_fp64| / cell = 1.100e-05 (torus_9x9x5), 3.943e-07 for the
3841 records in one cell; blob32 at 8 cells: 2844 -> 264 faces, output within 0.165 D of the input, |w - rint(w)| <= 9.1e-08."""
import ctypes as C

import numpy as np
import pytest
import torch

import iso_cases as I
import mesh_simplify_oracle as O
from test_mesh_simplify_host import load_host, position_error, simplify as host_simplify

pytestmark = pytest.mark.gpu

GATE = O.GATE


@pytest.fixture(scope='module')
def dsdf(built):
    import dsdf as m
    m.load()
    assert torch.cuda.is_available()
    return m


@pytest.fixture(scope='module')
def host():
    return load_host()


def _cuda(a, dt=None):
    return torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()


def device_simplify(dsdf, v, f, box, cells, colors=None, **kw):
    out = dsdf.simplify_mesh(_cuda(v, np.float32), _cuda(f, np.int32), cells, bounds=box, normals=True,
                             colors=None if colors is None else _cuda(colors, np.float32), **kw)
    assert out[0].dtype == torch.float32 and out[1].dtype == torch.int32 and out[0].shape[1:] == (3,) and out[1].shape[1:] == (3,)
    keys = ('vertices', 'faces', 'normals', 'colors')
    return {k: t.cpu().numpy() for k, t in zip(keys, out)}


def assert_same_bits(dev, hst, what):
    for k in ('faces', 'vertices', 'normals', 'colors'):
        if hst.get(k) is None:
            continue
        assert dev[k].shape == hst[k].shape, (what, k, dev[k].shape, hst[k].shape)
        assert np.array_equal(dev[k].view(np.int32), hst[k].view(np.int32)), (what, k)


# ---- 1, 2. every case of the table: the host's bits, the reference within the gate -----------------------------------------------------
@pytest.mark.parametrize('name', list(O.CASES))
def test_device_equals_host_build_and_matches_fp64(dsdf, host, name):
    mname, box, cells = O.CASES[name]
    v, f = O.mesh(mname)
    col = O.colors_of(v)
    dev = device_simplify(dsdf, v, f, box, cells, colors=col)
    assert_same_bits(dev, host_simplify(host, v, f, box[0], box[1], cells, colors=col), name)
    ref = O.reference(name)
    assert np.array_equal(dev['faces'], ref['faces']) and dev['vertices'].shape == ref['vertices'].shape
    err = position_error(dev, ref, box, cells)
    print(f'{name}: {len(f)} -> {len(dev["faces"])} faces; device max |x_fp32 - x_fp64| / cell = {err:.3e}')
    assert err <= GATE
    if len(ref['vertices']):
        assert np.abs(dev['normals'] - ref['normals']).max() <= GATE and np.abs(dev['colors'] - ref['colors']).max() <= GATE
    # the optional outputs change nothing else
    plain = dsdf.simplify_mesh(_cuda(v, np.float32), _cuda(f, np.int64), cells, bounds=box)
    assert len(plain) == 2 and np.array_equal(plain[0].cpu().numpy(), dev['vertices']) and np.array_equal(plain[1].cpu().numpy(), dev['faces'])


# ---- 3. sizes that cross launch boundaries ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_faces', [255, 256, 257])
def test_face_counts_around_one_block(dsdf, host, n_faces):
    v, f = O.mesh('sphere')
    f = f[:n_faces]
    dev = device_simplify(dsdf, v, f, O.UNIT, (9, 9, 9), colors=O.colors_of(v))
    hst = host_simplify(host, v, f, O.UNIT[0], O.UNIT[1], (9, 9, 9), colors=O.colors_of(v))
    assert 0 < len(hst['faces']) < n_faces
    assert_same_bits(dev, hst, n_faces)


def ribbon(n):
    """Two rows of 3 n vertices, three per cell of an (n, 2, 1) grid of CUBIC cells of size 1 / n over the box [0, 1] x [0, 2 / n] x
    [0, 1 / n]: 2 n occupied cells, all of them used.  -> (vertices, faces, box)"""
    m = 3 * n
    x = (np.arange(m) + 0.5) / m
    rows = [np.stack([x, np.full(m, y / n), (0.5 + 0.3 * np.sin(2.1 * n * x + y)) / n], -1) for y in (0.6, 1.6)]
    v = np.concatenate(rows).astype(np.float32)
    faces = []
    for j in range(m - 1):
        faces += [(j, j + 1, m + j), (j + 1, m + j + 1, m + j)]
    return v, np.asarray(faces, np.int64), ((0.0, 0.0, 0.0), (1.0, 2.0 / n, 1.0 / n))


@pytest.mark.parametrize('n', [32, 33, 128, 129], ids=lambda n: f'{2 * n}cells')
def test_occupied_cell_counts_around_64_and_256(dsdf, host, n):
    v, f, box = ribbon(n)
    cells = (n, 2, 1)
    hst = host_simplify(host, v, f, box[0], box[1], cells, colors=O.colors_of(v))
    assert hst['occupied'] == 2 * n and hst['vertices'].shape == (2 * n, 3) and len(hst['faces']) == 2 * (n - 1)
    assert_same_bits(device_simplify(dsdf, v, f, box, cells, colors=O.colors_of(v)), hst, n)
    ref = O.simplify(v, f, box[0], box[1], cells)
    assert np.array_equal(hst['faces'], ref['faces']) and position_error(hst, ref, box, cells) <= GATE


def test_one_cell_with_every_corner_of_1280_faces(dsdf, host):
    """The longest segment loop: all 3840 corners of the sphere in ONE cell, which one more face reaching into two other cells keeps in use."""
    v, f = O.mesh('sphere')
    v = np.concatenate([v, np.float32([[1.0, 0.1, 0.0], [0.1, 1.0, 0.0]])])
    f = np.concatenate([f, [[0, len(v) - 2, len(v) - 1]]])
    box, cells = ((-0.5, -0.5, -0.5), (1.5, 1.5, 0.5)), (2, 2, 1)
    hst = host_simplify(host, v, f, box[0], box[1], cells, colors=O.colors_of(v))
    assert hst['occupied'] == 3 and hst['vertices'].shape == (3, 3) and np.array_equal(hst['faces'], [[0, 1, 2]])
    assert_same_bits(device_simplify(dsdf, v, f, box, cells, colors=O.colors_of(v)), hst, 'one cell')
    ref = O.simplify(v, f, box[0], box[1], cells)
    err = position_error(hst, ref, box, cells)
    print(f'3841 records in one cell: max |x_fp32 - x_fp64| / cell = {err:.3e}')
    assert err <= GATE


def test_no_faces_and_everything_collapsed(dsdf):
    v, f = O.mesh('sphere')
    for faces, colors in ((f[:0], None), (f[:0], O.colors_of(v)), (f, O.colors_of(v))):
        out = dsdf.simplify_mesh(_cuda(v), _cuda(faces, np.int32), 1, bounds=O.UNIT, normals=True, colors=None if colors is None else _cuda(colors))
        assert len(out) == (3 if colors is None else 4)
        assert all(tuple(t.shape) == (0, 3) and t.is_cuda for t in out) and out[1].dtype == torch.int32
    out = dsdf.simplify_mesh(torch.zeros(0, 3, device='cuda'), torch.zeros(0, 3, dtype=torch.int32, device='cuda'), 4)
    assert len(out) == 2 and all(tuple(t.shape) == (0, 3) for t in out)
    lib = dsdf.load()
    lo, hi = (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, 1, 1)
    assert lib.dsdf_simplify_keys(None, None, 0, lo, hi, 4, 4, 4, None, None) == 0         # F = 0: no launch, no pointers
    assert lib.dsdf_simplify_mark(None, 0, None, 0, None, None, None, None) == 0
    assert lib.dsdf_simplify_emit(None, None, 0, None, lo, hi, 4, 4, 4, C.c_float(1e-3), *([None] * 3), 0, *([None] * 10)) == 0


# ---- 6. the guarantees through the product's own queries ---------------------------------------------------------------------------------
def test_guarantees_on_an_extracted_mesh(dsdf):
    """blob32 extracted at its own resolution and simplified at 8 cells.  1: dsdf.mesh_distance from the output to the input stays
    within one cell diagonal D.  2: dsdf.mesh_winding of both at the points farther than D from the input rounds to the same integer.
    The sum of T fp32 terms below 1/2 each, of partial sums within [-1, 2], is off by at most about T 2^-23 (1e-3 at T = 1e4):
    the bound on |w - rint(w)| here."""
    grid = dsdf.SdfGrid(torch.from_numpy(I.grid('blob32')).float().cuda())
    v, f, n = dsdf.extract_mesh(grid)
    lo, hi = v.amin(0).double(), v.amax(0).double()
    g = 2.0 ** -13 * float((hi - lo).max())
    lo, hi = (lo - g).float().tolist(), (hi + g).float().tolist()
    cells = dsdf.renderer.resolve_cells(8, lo, hi)
    assert max(cells) == 8 and min(cells) >= 1
    vs, fs, ns = dsdf.simplify_mesh(v, f, cells, bounds=(lo, hi), normals=True)
    again = dsdf.simplify_mesh(v, f, 8, normals=True)                                   # the default box is this box
    assert all(torch.equal(a, b) for a, b in zip((vs, fs, ns), again))
    assert 0 < fs.shape[0] < f.shape[0] // 4 and vs.shape[0] < v.shape[0] // 4
    D = O.diagonal(lo, hi, cells)
    tri_in, tri_out = v[f.long()], vs[fs.long()]
    d = dsdf.mesh_distance(tri_out, tri_in, n=20000)
    print(f'blob32: {f.shape[0]} -> {fs.shape[0]} faces at {cells} cells; output -> input max {d["a_to_b_max"] / D:.3f} D, '
          f'input -> output max {d["b_to_a_max"] / D:.3f} D')
    assert d['a_to_b_max'] <= D + GATE * D
    assert float((ns.norm(dim=1) - 1).abs().max()) < 1e-5                                # unit normals: no cell's normal sum vanishes here
    pts = torch.rand(4000, 3, device='cuda', generator=torch.Generator(device='cuda').manual_seed(1)) * 1.4 - 0.2
    far = dsdf.MeshBvh(tri_in).closest(pts) > D
    pts = pts[far].contiguous()
    assert pts.shape[0] >= 200
    w_in, w_out = dsdf.mesh_winding(tri_in, pts), dsdf.mesh_winding(tri_out, pts)
    tol = max(f.shape[0] * 2.0 ** -23, 1e-4)
    print(f'blob32: {pts.shape[0]} points farther than D = {D:.3f}; max |w_in - rint| = {float((w_in - w_in.round()).abs().max()):.2e}, '
          f'max |w_out - rint| = {float((w_out - w_out.round()).abs().max()):.2e} (bound {tol:.1e})')
    assert float((w_in - w_in.round()).abs().max()) < tol, 'the extracted mesh is not closed'
    assert torch.equal(w_in.round(), w_out.round()) and float((w_out - w_out.round()).abs().max()) < tol


# ---- 7. the command lines ------------------------------------------------------------------------------------------------------------------
def test_extract_mesh_cli_with_simplify(dsdf, tmp_path):
    import extract_mesh
    import mesh_to_sdf
    import util
    import test_gpu_mesh_render as T
    data = torch.from_numpy(I.grid('sphere16')).float()
    alb = T.albedo_volume()
    util.write_vol(str(tmp_path / 'sdf.vol'), data)
    util.write_vol(str(tmp_path / 'albedo.vol'), alb)
    out = str(tmp_path / 'out.ply')
    assert extract_mesh.main([str(tmp_path / 'sdf.vol'), '--albedo', str(tmp_path / 'albedo.vol'), '--float-colors', '--simplify', '6', '-o', out]) == 0
    v, f, c = mesh_to_sdf.load_mesh_indexed(out, colors=True)
    full = dsdf.extract_mesh(dsdf.SdfGrid(data.cuda()), colors=util.read_vol(str(tmp_path / 'albedo.vol')).float().contiguous().cuda())
    want = dsdf.simplify_mesh(full[0], full[1], 6, normals=True, colors=full[3])
    assert 0 < len(f) < full[1].shape[0] and c is not None
    assert np.array_equal(v, want[0].cpu().numpy()) and np.array_equal(f, want[1].cpu().numpy()) and np.array_equal(c, want[3].cpu().numpy())
    plain = str(tmp_path / 'plain.ply')
    assert extract_mesh.main([str(tmp_path / 'sdf.vol'), '-o', plain]) == 0           # without --simplify: what it was
    assert np.array_equal(mesh_to_sdf.load_mesh_indexed(plain)[1], full[1].cpu().numpy())
    with pytest.raises(SystemExit) as e:
        extract_mesh.main([str(tmp_path / 'sdf.vol'), '--simplify', '0', '-o', out])
    assert e.value.code not in (0, None)


@pytest.mark.parametrize('ext', ['ply', 'obj'])
def test_simplify_mesh_cli_round_trip_with_colors(dsdf, tmp_path, ext):
    import mesh_to_sdf
    import simplify_mesh
    v, f = O.mesh('torus')
    col = O.colors_of(v)
    src, out = str(tmp_path / f'in.{ext}'), str(tmp_path / f'out.{ext}')
    if ext == 'ply':
        mesh_to_sdf.save_ply(src, v, f, colors=col, color_dtype='float')
    else:
        mesh_to_sdf.save_obj(src, v, f, colors=col)
    assert simplify_mesh.main([src, out, '--cells', '9'] + (['--float-colors'] if ext == 'ply' else [])) == 0
    v_in, f_in, c_in = mesh_to_sdf.load_mesh_indexed(src, colors=True)
    want = dsdf.simplify_mesh(_cuda(v_in, np.float32), _cuda(f_in, np.int32), 9, normals=True, colors=_cuda(c_in, np.float32))
    v2, f2, c2 = mesh_to_sdf.load_mesh_indexed(out, colors=True)
    assert 0 < len(f2) < len(f) and c2 is not None and c2.shape == v2.shape
    assert np.array_equal(v2, want[0].cpu().numpy()) and np.array_equal(f2, want[1].cpu().numpy())
    assert np.array_equal(c2, want[3].cpu().numpy())
    # without colours in the file none are written
    mesh_to_sdf.save_ply(str(tmp_path / 'bare.ply'), v, f)
    assert simplify_mesh.main([str(tmp_path / 'bare.ply'), str(tmp_path / 'bare_out.ply'), '--cells', '9']) == 0
    assert mesh_to_sdf.load_mesh_indexed(str(tmp_path / 'bare_out.ply'), colors=True)[2] is None


# ---- 8. argument validation ---------------------------------------------------------------------------------------------------------------
def test_argument_validation(dsdf):
    lib = dsdf.load()
    one = C.c_void_p(16)            # never dereferenced: validation fails first
    lo, hi = (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, 1, 1)
    flat_hi = (C.c_float * 3)(1, 0, 1)
    reg = C.c_float(1e-3)

    def keys(v=one, f=one, F=8, lo=lo, hi=hi, c=(4, 4, 4), out=one):
        return lib.dsdf_simplify_keys(v, f, F, lo, hi, c[0], c[1], c[2], out, None)

    def mark(k=one, F=8, ck=one, U=4, r=one, keep=one, used=one):
        return lib.dsdf_simplify_mark(k, F, ck, U, r, keep, used, None)

    def emit(v=one, f=one, F=8, col=None, lo=lo, hi=hi, c=(4, 4, 4), reg=reg, corner=one, U=4, pos=one, col_out=None):
        return lib.dsdf_simplify_emit(v, f, F, col, lo, hi, c[0], c[1], c[2], reg, corner, one, one, U, one, one, one, one, one, one, pos, None, col_out, None)
    grid_bad = [dict(c=(2048, 1024, 1024)), dict(c=(65536, 65536, 1)), dict(c=(4, 0, 4)), dict(hi=flat_hi), dict(lo=None), dict(hi=None)]
    for call, name, bad in ((keys, b'dsdf_simplify_keys', grid_bad + [dict(v=None), dict(f=None), dict(out=None), dict(F=-1), dict(F=1 << 30)]),
                            (mark, b'dsdf_simplify_mark', [dict(k=None), dict(ck=None), dict(r=None), dict(keep=None), dict(used=None), dict(F=-1), dict(U=0)]),
                            (emit, b'dsdf_simplify_emit', grid_bad + [dict(v=None), dict(f=None), dict(corner=None), dict(pos=None), dict(U=0), dict(F=-1),
                                                                      dict(reg=C.c_float(0.0)), dict(reg=C.c_float(float('nan'))), dict(col_out=one)])):
        for kw in bad:
            assert call(**kw) == -1 and lib.dsdf_last_error().startswith(name), (name, kw, lib.dsdf_last_error())
    assert keys(F=0, c=(2048, 1024, 1024)) == -1 and b'2^31' in lib.dsdf_last_error()          # refused before anything else, F = 0 included
    v, f = (_cuda(a, dt) for a, dt in zip(O.mesh('sphere'), (np.float32, np.int32)))
    with pytest.raises(dsdf.DsdfError, match='no CPU path'):
        dsdf.simplify_mesh(v.cpu(), f.cpu(), 4)
    with pytest.raises(dsdf.DsdfError, match='no CPU path'):
        dsdf.simplify_mesh(v, f.cpu(), 4)
    with pytest.raises(dsdf.DsdfError, match=r'\(V,3\)'):
        dsdf.simplify_mesh(v.reshape(-1), f, 4)
    with pytest.raises(dsdf.DsdfError, match=r'\(F,3\)'):
        dsdf.simplify_mesh(v, f.reshape(-1), 4)
    with pytest.raises(dsdf.DsdfError, match='float32'):
        dsdf.simplify_mesh(v.double(), f, 4)
    with pytest.raises(dsdf.DsdfError, match='int32'):
        dsdf.simplify_mesh(v, f.float(), 4)
    with pytest.raises(dsdf.DsdfError, match='out of range'):
        dsdf.simplify_mesh(v[:100], f, 4)
    with pytest.raises(dsdf.DsdfError, match='out of range'):
        dsdf.simplify_mesh(v, f - 1, 4)
    with pytest.raises(dsdf.DsdfError, match='colors'):
        dsdf.simplify_mesh(v, f, 4, colors=v[:10])
    for reg_bad in (0.0, -1.0, float('nan')):
        with pytest.raises(dsdf.DsdfError, match='reg'):
            dsdf.simplify_mesh(v, f, 4, reg=reg_bad)
    with pytest.raises(dsdf.DsdfError, match='cells'):
        dsdf.simplify_mesh(v, f, 0)
    with pytest.raises(dsdf.DsdfError, match='dsdf_simplify_keys.*2\\^31'):
        dsdf.simplify_mesh(v, f, (2048, 1024, 1024))
    with pytest.raises(dsdf.DsdfError, match='dsdf_simplify_keys.*lo < hi'):
        dsdf.simplify_mesh(v, f, 4, bounds=((0, 0, 0), (1, 0, 1)))
    # one shared box puts two meshes on one grid: the part of the sphere is simplified as it is within the whole
    whole = dsdf.simplify_mesh(v, f, 6, bounds=O.UNIT)
    part = dsdf.simplify_mesh(v, f[:400], 6, bounds=O.UNIT)
    assert 0 < part[1].shape[0] < whole[1].shape[0]
