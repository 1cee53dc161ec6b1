"""GPU check of the surface extraction (include/dsdf.h: dsdf_iso_*, dsdf.extract_mesh) against the numpy oracle of tests/iso_cases.py:
mark + emit on value lattices uploaded as they are EQUAL the oracle's outputs; on grids the sampled values agree with the fp64 lookup,
the topology equals the oracle run on the GPU's own values, the vertices lie on the rendered surface and the normals follow its
gradient; the extracted mesh, rendered through dsdf.MeshBvh, reproduces the SDF render."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import iso_cases as I
import mesh_render_oracle as R
import sdf_oracle as O
from iso_cases import ON_EDGE_TOL, VERTEX_RESIDUAL_GATE, assert_same_topology

pytestmark = pytest.mark.gpu

W = H = 24
SPP = 8


@pytest.fixture(scope='module')
def dsdf(built):
    import dsdf as m
    m.load()
    assert torch.cuda.is_available()
    return m


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def gpu_topology(dsdf, values, n, iso=0.0):
    """dsdf_iso_mark, the two scans, dsdf_iso_emit on a device buffer of values -> numpy outputs."""
    lib = dsdf.load()
    N = I.n_nodes(n)
    assert values.numel() == N
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    cross = torch.full((N,), 255, dtype=torch.uint8, device='cuda')
    nv = torch.full((N,), -1, dtype=torch.int32, device='cuda'); nt = torch.full((N,), -1, dtype=torch.int32, device='cuda')
    assert lib.dsdf_iso_mark(_ptr(values), *n, C.c_float(iso), _ptr(cross), _ptr(nv), _ptr(nt), st) == 0, lib.dsdf_last_error()
    vo = (torch.cumsum(nv, 0) - nv).to(torch.int32); to = (torch.cumsum(nt, 0) - nt).to(torch.int32)
    V, F = int(nv.sum()), int(nt.sum())
    ve = torch.full((max(V, 1),), -1, dtype=torch.int32, device='cuda'); faces = torch.full((max(F, 1), 3), -1, dtype=torch.int32, device='cuda')
    assert lib.dsdf_iso_emit(_ptr(values), *n, C.c_float(iso), _ptr(cross), _ptr(vo), _ptr(to), _ptr(ve), _ptr(faces), st) == 0, lib.dsdf_last_error()
    return dict(cross=cross.cpu().numpy(), n_vert=nv.cpu().numpy(), n_tri=nt.cpu().numpy(), vert_edge=ve[:V].cpu().numpy(),
                faces=faces[:F].cpu().numpy())


@pytest.mark.parametrize('name', list(I.VALUE_LATTICES))
def test_mark_and_emit_on_value_lattices(dsdf, name):
    n, values = I.VALUE_LATTICES[name]
    got = gpu_topology(dsdf, torch.from_numpy(values).cuda(), n)
    assert_same_topology(got, I.topology(values, n), name)


def sdf_grid(dsdf, name):
    return dsdf.SdfGrid(torch.from_numpy(I.grid(name)).float().cuda())


GRID_RUNS = [('sphere16', (16, 16, 16)), ('sphere16', (17, 16, 15)), ('blob32_24', (32, 32, 32))]


@pytest.mark.parametrize('name,n', GRID_RUNS, ids=[f'{a}-{"x".join(map(str, b))}' for a, b in GRID_RUNS])
def test_extraction_on_grids(dsdf, name, n):
    lib = dsdf.load()
    grid = sdf_grid(dsdf, name)
    data = I.grid(name)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    values = torch.full((I.n_nodes(n),), float('nan'), dtype=torch.float32, device='cuda')
    assert lib.dsdf_iso_sample(_ptr(grid.padded), grid.rx, grid.ry, grid.rz, *n, _ptr(values), st) == 0, lib.dsdf_last_error()
    ref64 = I.oracle_values(data, n)
    vh = values.cpu().numpy()
    e = np.linalg.norm(vh - ref64) / np.linalg.norm(ref64)
    print(f'{name} {n}: values rel-L2 {e:.3e}, smallest |value| {np.abs(vh).min():.3e}')
    assert e < 1e-6
    # the topology is the oracle's on the GPU's own values ...
    ref = I.topology(vh, n)
    assert_same_topology(gpu_topology(dsdf, values, n), ref, (name, n))
    # ... and what extract_mesh returns
    v, f, nrm = dsdf.extract_mesh(grid, resolution=n)
    assert v.dtype == torch.float32 and f.dtype == torch.int32 and v.is_cuda and f.is_cuda and nrm.shape == v.shape
    assert np.array_equal(I.canonical_faces(f.cpu().numpy()), I.canonical_faces(ref['faces'])) and v.shape[0] == len(ref['vert_edge'])
    # vertices: on their edges, on the surface (the gate of the host test)
    a, b, _ = I.edge_endpoints(ref['vert_edge'], n)
    pos = v.cpu().numpy().astype(np.float64)
    d = b - a
    s = ((pos - a) * d).sum(1) / (d * d).sum(1)
    off = np.linalg.norm(pos - (a + np.clip(s, 0.0, 1.0)[:, None] * d), axis=1)
    assert off.max() <= ON_EDGE_TOL, off.max()
    res = np.abs(I.f64(data, pos)).max()
    # normals
    nh = nrm.cpu().numpy().astype(np.float64)
    _, g = I.f64(data, pos, 1)
    g /= np.linalg.norm(g, axis=1, keepdims=True)
    en = np.linalg.norm(nh - g) / np.linalg.norm(g)
    print(f'{name} {n}: {len(pos)} vertices, {len(ref["faces"])} faces, max |f64(vertex)| {res:.3e} (gate {VERTEX_RESIDUAL_GATE:.3e}), normals rel-L2 {en:.3e}')
    assert res <= VERTEX_RESIDUAL_GATE, res
    assert np.abs(np.linalg.norm(nh, axis=1) - 1).max() < 1e-6
    assert en < 1e-5, en


@functools.lru_cache(maxsize=None)
def view():
    import dsdf
    sensor = dsdf.get_regular_cameras(3, resx=W, resy=H)[1]
    cam = O.Camera.from_params(np.frombuffer(bytes(sensor.to_struct()), np.float32, 16))
    offsets = torch.rand((W + 4) * (H + 4) * SPP, 2, generator=torch.Generator().manual_seed(7))
    return sensor, cam, offsets


@functools.lru_cache(maxsize=None)
def oracle_distance(n, p=(0.0, 0.0, 0.0)):
    """d(n) of the fp64 reference: its mesh render of the oracle's fp64 mesh against its SDF render, mean absolute difference."""
    _, cam, offsets = view()
    m = I.oracle_mesh_of('sphere16', (n, n, n))
    tri = (m['positions'] + np.asarray(p))[m['faces']]
    mesh_img = R.render(tri, m['normals'][m['faces']], cam, W, H, SPP, offsets, O.SILHOUETTE)
    sdf = O.Grid3d(torch.from_numpy(I.grid('sphere16')), p=torch.tensor(p, dtype=torch.float64))
    sdf_img = O.render(sdf, cam, W, H, SPP, offsets.double(), integrator=O.SILHOUETTE, reparam=False).detach().numpy()
    return float(np.abs(mesh_img - sdf_img).mean())


def gpu_distance(dsdf, grid, n):
    sensor, _, offsets = view()
    v, f, nrm = dsdf.extract_mesh(grid, resolution=n)
    bvh = dsdf.MeshBvh(v[f.long()], nrm[f.long()])
    off = offsets[None].cuda()
    mesh_img = dsdf.mesh_render(bvh, [sensor], SPP, offsets=off, integrator=dsdf.DSDF_SILHOUETTE)
    sdf_img = dsdf.render_forward(grid, [sensor], SPP, offsets=off, integrator=dsdf.DSDF_SILHOUETTE, reparam=False)
    assert float(sdf_img.mean()) > 0.05                                       # the object is in the picture
    return float((mesh_img - sdf_img).abs().mean())


def test_round_trip_through_the_renderers(dsdf):
    """mesh_render(extract_mesh(sdf)) against render_forward(sdf): at n = 32 the GPU must not be further from its SDF render than the
    fp64 reference is at n = 16 (reference with these offsets: d(16) = 8.63e-4, d(32) = 0; measured on the MI355X: d(32) = 9.3e-9)."""
    grid = sdf_grid(dsdf, 'sphere16')
    d16_ref = oracle_distance(16)
    d32 = gpu_distance(dsdf, grid, 32)
    print(f'round trip: oracle d(16) = {d16_ref:.3e}, GPU d(32) = {d32:.3e}, GPU d(16) = {gpu_distance(dsdf, grid, 16):.3e}')
    assert d16_ref > 0 and d32 <= d16_ref, (d32, d16_ref)


def test_translation_moves_the_vertices(dsdf):
    """`sdf.p` is applied by the Python layer: the vertices move by exactly p (in fp32), the faces stay, the round trip still passes."""
    grid = sdf_grid(dsdf, 'sphere16')
    v0, f0, n0 = dsdf.extract_mesh(grid, resolution=16)
    p = (0.0625, -0.03125, 0.125)
    grid.set_translation(p)
    v1, f1, n1 = dsdf.extract_mesh(grid, resolution=16)
    assert torch.equal(f0, f1) and torch.equal(n0, n1)
    assert torch.equal(v1, v0 + torch.tensor(p, device='cuda'))
    d32 = gpu_distance(dsdf, grid, 32)
    d16_ref = oracle_distance(16, p)
    print(f'translated round trip: oracle d(16) = {d16_ref:.3e}, GPU d(32) = {d32:.3e}')
    assert d16_ref > 0 and d32 <= d16_ref, (d32, d16_ref)


def test_general_transform_maps_vertices_and_normals(dsdf):
    """A grid with a general to_world: vertices through to_world (+ p), normals through its inverse transpose."""
    data = torch.from_numpy(I.grid('sphere16')).float().cuda()
    v0, f0, n0 = dsdf.extract_mesh(dsdf.SdfGrid(data), resolution=16)
    c, s = np.cos(0.4), np.sin(0.4)
    tw = np.array([[1.2 * c, -s, 0, 0.1], [1.2 * s, c, 0, -0.05], [0, 0, 0.9, 0.2], [0, 0, 0, 1]])
    grid = dsdf.SdfGrid(data, to_world=tw).set_translation((0.01, 0.02, 0.03))
    v1, f1, n1 = dsdf.extract_mesh(grid, resolution=16)
    assert torch.equal(f0, f1)
    want_v = v0.double().cpu().numpy() @ tw[:3, :3].T + tw[:3, 3] + np.array([0.01, 0.02, 0.03])
    want_n = n0.double().cpu().numpy() @ np.linalg.inv(tw[:3, :3])
    want_n /= np.linalg.norm(want_n, axis=1, keepdims=True)
    assert np.abs(v1.cpu().numpy() - want_v).max() < 1e-6 and np.abs(n1.cpu().numpy() - want_n).max() < 1e-6
    # the mapped normal is the gradient direction of the transformed field: it agrees with the library's world-space lookup
    _, g, _ = dsdf.eval_cubic(grid, v1, order=1)
    g = torch.nn.functional.normalize(g, dim=1)
    assert float((g - n1).abs().max()) < 1e-4


def test_empty_surface(dsdf):
    grid = dsdf.SdfGrid(torch.full((8, 8, 8), 0.5, device='cuda'))
    v, f, n = dsdf.extract_mesh(grid)
    assert tuple(v.shape) == (0, 3) and tuple(f.shape) == (0, 3) and tuple(n.shape) == (0, 3)
    v, f = dsdf.extract_mesh(grid, resolution=(3, 4, 5), normals=False)
    assert tuple(v.shape) == (0, 3) and tuple(f.shape) == (0, 3) and f.dtype == torch.int32
    with pytest.raises(dsdf.DsdfError, match='dsdf_iso_sample'):
        dsdf.extract_mesh(grid, resolution=0)
    with pytest.raises(dsdf.DsdfError, match='steps must be'):
        dsdf.extract_mesh(sdf_grid(dsdf, 'sphere16'), steps=40)
