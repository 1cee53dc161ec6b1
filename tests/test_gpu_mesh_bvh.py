"""GPU checks of the mesh BVH (csrc/dsdf_bvh.h): dsdf_mesh_bvh_raycast returns BITWISE what the brute-force dsdf_mesh_raycast
returns, the built buffer has the documented structure, the ray casts match the fp64 oracle like the brute-force ones do, and
`create_sdf` does not depend on the path its rays take."""
import numpy as np
import pytest
import torch

import mesh_oracle as M
from mesh_bvh_cases import MESHES, n_leaves, ray_sets
from mesh_render_oracle import locate

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dsdf(built):
    import dsdf as m
    m.load()
    assert torch.cuda.is_available()
    return m


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize('name', list(MESHES))
def test_bvh_raycast_is_bitwise_brute_force(dsdf, name):
    tri = MESHES[name]
    tri_d = _cuda(tri)
    bvh = dsdf.MeshBvh(tri_d)
    sets = ray_sets(tri, len(name))
    rng = np.random.default_rng(5000)
    d5 = rng.normal(size=(5000, 3))
    sets['n5000'] = (rng.uniform(-0.5, 0.5, (5000, 3)).astype(np.float32), (d5 / np.linalg.norm(d5, axis=1, keepdims=True)).astype(np.float32), 0.0)
    for rs, (o, d, t_min) in sets.items():
        od, dd = _cuda(o), _cuda(d)
        t, back, prim = bvh.raycast(od, dd, t_min=t_min, return_prim=True)
        t_ref, back_ref = dsdf.mesh_raycast(tri_d, od, dd, t_min=t_min)
        assert t.shape == (o.shape[0],) and prim.dtype == torch.int32
        assert torch.equal(t.view(torch.int32), t_ref.view(torch.int32)), (name, rs)
        assert torch.equal(back, back_ref), (name, rs)
        t, prim = t.cpu().numpy(), prim.cpu().numpy()
        assert ((prim >= 0) == np.isfinite(t)).all() and (prim < tri.shape[0]).all()
        if o.shape[0] and (tri.shape[0] <= 400 or rs == 'random'):
            # the primitive: fp64 argmin over all triangles, on rays whose winner is unique (the largest mesh: one ray set)
            t64, k64, _, _ = locate(tri, o, d, t_min, block=256)
            _, _, margin = M.raycast(tri, o, d, t_min, block=256)
            sure = (margin > 1e-4) & np.isfinite(t64) & np.isfinite(t)
            sure &= np.abs(np.where(sure, t - t64, 0.0)) <= 2e-5 * np.abs(np.where(sure, t64, 0.0)) + 2e-6     # (the same hit in both precisions)
            assert (prim[sure] == k64[sure]).all(), (name, rs)


@pytest.mark.parametrize('name', ['T1', 'T5', 'box12', 'ico320', 'ico5120', 'zero_area'])
@pytest.mark.parametrize('with_normals', [False, True])
def test_buffer_structure(dsdf, name, with_normals):
    tri = MESHES[name]
    T, L = tri.shape[0], n_leaves(tri.shape[0])
    nrm = np.random.default_rng(1).normal(size=tri.shape).astype(np.float32) if with_normals else None
    bvh = dsdf.MeshBvh(_cuda(tri), None if nrm is None else _cuda(nrm))
    buf = bvh.buffer.cpu().numpy()
    assert buf.size == L * (100 if with_normals else 64)
    ints = buf.view(np.int32)
    assert (ints[0], ints[1], ints[2]) == (T, L, int(with_normals))
    np.testing.assert_array_equal(buf[4:7], tri.reshape(-1, 3).min(0)); np.testing.assert_array_equal(buf[7:10], tri.reshape(-1, 3).max(0))
    slots = buf[16 * L:64 * L].reshape(4 * L, 12)
    idx = slots.view(np.int32)[:, 9]
    assert sorted(idx[:T].tolist()) == list(range(T)) and (idx[T:] == -1).all()       # a permutation, then empty slots
    np.testing.assert_array_equal(slots[:T, :9], tri.reshape(T, 9)[idx[:T]])
    if with_normals:
        np.testing.assert_array_equal(buf[64 * L:100 * L].reshape(4 * L, 9)[:T], nrm.reshape(T, 9)[idx[:T]])
    if L == 1:
        return
    # boxes of all heap nodes i >= 1, read from their parents
    nodes = buf[16:16 * L].reshape(L - 1, 16)
    lo = np.zeros((2 * L - 1, 3), np.float32); hi = np.zeros((2 * L - 1, 3), np.float32)
    for i in range(1, 2 * L - 1):
        b = nodes[(i - 1) // 2, 6 * ((i - 1) & 1):6 * ((i - 1) & 1) + 6]
        lo[i], hi[i] = b[:3], b[3:]
    for j in range(L):
        i = L - 1 + j
        own = slots[4 * j:4 * j + 4][idx[4 * j:4 * j + 4] >= 0, :9].reshape(-1, 3)
        if own.size == 0:
            assert (lo[i] == np.inf).all() and (hi[i] == -np.inf).all()               # empty leaves are inverted
        else:
            assert (own >= lo[i]).all() and (own <= hi[i]).all()                      # every triangle lies inside its leaf box
    for i in range(1, L - 1):
        for c in (2 * i + 1, 2 * i + 2):
            if (lo[c] <= hi[c]).all():                                                # (an empty child lies inside anything)
                assert (lo[c] >= lo[i]).all() and (hi[c] <= hi[i]).all()              # every child box lies inside its parent's


@pytest.mark.parametrize('n_rays', [1, 63, 5000])
def test_bvh_raycast_matches_oracle(dsdf, n_rays):
    """The gate of test_gpu_mesh_to_sdf.py::test_raycast_matches_oracle, through the BVH."""
    v, f = M.icosphere(0.3, 2, centre=(0.05, -0.02, 0.01))
    tri = v[f]
    rng = np.random.default_rng(n_rays)
    o = rng.uniform(-0.5, 0.5, (n_rays, 3)).astype(np.float32)
    d = rng.normal(size=(n_rays, 3)); d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    t_ref, back_ref, margin = M.raycast(tri, o, d)
    t, back = dsdf.MeshBvh(_cuda(tri)).raycast(_cuda(o), _cuda(d))
    t, back = t.cpu().numpy(), back.cpu().numpy()
    sure = margin > 1e-4
    assert sure.mean() > 0.95
    assert (np.isfinite(t) == np.isfinite(t_ref))[sure].all()
    hit = sure & np.isfinite(t_ref)
    np.testing.assert_allclose(t[hit], t_ref[hit], rtol=2e-5, atol=2e-6)
    assert (back[hit] != 0).tolist() == back_ref[hit].tolist()


@pytest.mark.parametrize('shape', ['box', 'sphere'])
def test_create_sdf_does_not_depend_on_the_path(dsdf, shape):
    import mesh_to_sdf
    v, f = M.box() if shape == 'box' else M.icosphere(0.3, 2)
    a = mesh_to_sdf.create_sdf(v[f], 16, accel='bvh')
    b = mesh_to_sdf.create_sdf(v[f], 16, accel='brute')
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    with pytest.raises(ValueError):
        mesh_to_sdf.create_sdf(v[f], 16, accel='octree')


def test_raycast_validation_and_empty(dsdf):
    import ctypes as C
    lib = dsdf.load()
    one = C.c_void_p(16)
    assert lib.dsdf_mesh_bvh_size(0, 0) == 0 and lib.dsdf_mesh_bvh_size(5, 0) == 128 and lib.dsdf_mesh_bvh_size(5, 1) == 200
    assert lib.dsdf_mesh_bvh_raycast(None, one, one, 4, C.c_float(0), one, None, None, None) == -1
    assert b'dsdf_mesh_bvh_raycast' in lib.dsdf_last_error()
    assert lib.dsdf_mesh_bvh_build(None, None, None, 4, one, None) == -1 and b'dsdf_mesh_bvh_build' in lib.dsdf_last_error()
    assert lib.dsdf_mesh_morton(one, 0, one, None) == -1 and b'dsdf_mesh_morton' in lib.dsdf_last_error()
    bvh = dsdf.MeshBvh(_cuda(MESHES['box12']))
    e = torch.zeros(0, 3, device='cuda')
    t, back, prim = bvh.raycast(e, e, return_prim=True)
    assert t.numel() == 0 and back.numel() == 0 and prim.numel() == 0
