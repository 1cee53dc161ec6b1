"""GPU check of the brute-force mesh kernels (csrc/dsdf_mesh.h, csrc/dsdf_winding.h: k_mesh_raycast, k_mesh_closest, k_mesh_winding) at the
edges of their LDS tile of 256 triangles (mesh_for_each_triangle): one triangle, one short of a tile, a full tile, one over, two tiles,
two and one.  The meshes are the first T triangles of the 1280-triangle icosphere of the other mesh tests -- open surfaces, which is all
the same to these queries.  No new gate: the traversals must return the bits of the loops (rays, closest point) and both must match
the fp64 references within mesh_closest_oracle.GATE / mesh_winding_oracle.GATE."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import mesh_closest_oracle as CO
import mesh_oracle as M
import mesh_winding_oracle as WO
from mesh_bvh_cases import ray_sets

pytestmark = pytest.mark.gpu

SIZES = (1, 255, 256, 257, 512, 513)
RAY_SETS = ('random', 'axis', 't_min')


@pytest.fixture(scope='module')
def dsdf(built):
    import dsdf as m
    m.load()
    assert torch.cuda.is_available()
    return m


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def mesh(T):
    v, f = M.icosphere(0.3, 3, centre=(0.05, -0.02, 0.01))
    tri = np.ascontiguousarray(v[f][:T], np.float32)
    assert tri.shape == (T, 3, 3)
    return tri


def _bits(t):
    return t.view(torch.int32)


@pytest.mark.parametrize('T', SIZES)
def test_raycast_is_bitwise_the_traversal(dsdf, T):
    lib = dsdf.load()
    tri = mesh(T)
    tri_d = _cuda(tri)
    bvh = dsdf.MeshBvh(tri_d)
    sets = ray_sets(tri, T)
    hits = 0
    for rs in RAY_SETS:
        o, d, t_min = sets[rs]
        od, dd = _cuda(o), _cuda(d)
        t, back = dsdf.mesh_raycast(tri_d, od, dd, t_min=t_min)
        t_ref, back_ref = bvh.raycast(od, dd, t_min=t_min)
        assert torch.equal(_bits(t), _bits(t_ref)) and torch.equal(back, back_ref), (T, rs)
        # the C entry point without the back-face output
        t_only = torch.full_like(t, float('nan'))
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert lib.dsdf_mesh_raycast(tri_d.data_ptr(), T, od.data_ptr(), dd.data_ptr(), o.shape[0], C.c_float(t_min), t_only.data_ptr(), None, st) == 0
        assert torch.equal(_bits(t_only), _bits(t)), (T, rs)
        hits += int(torch.isfinite(t).sum())
    assert hits > 0                                                          # the rays do meet the mesh


@pytest.mark.parametrize('T', SIZES)
def test_closest_is_bitwise_the_traversal_and_matches_fp64(dsdf, T):
    tri = mesh(T)
    pts = CO.all_points(tri, T, n_random=2000)
    tri_d, pts_d = _cuda(tri), _cuda(pts)
    kw = dict(return_prim=True, return_point=True, return_bary=True)
    got = dsdf.mesh_closest(tri_d, pts_d, **kw)
    ref = dsdf.MeshBvh(tri_d).closest(pts_d, **kw)
    assert len(got) == len(ref) == 4
    for a, b in zip(got, ref):
        assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b)), T
    d64 = CO.closest(pts, tri)[0]
    err = np.abs(got[0].cpu().numpy().astype(np.float64) - d64).max()
    print(f'T = {T}: max |dist - dist_fp64| = {err:.3e}')
    assert err <= CO.GATE


@pytest.mark.parametrize('T', SIZES)
def test_winding_matches_fp64_and_the_exact_walk(dsdf, T):
    tri = mesh(T)
    pts = WO.all_points(tri, T, n_random=2000)
    finite = np.isfinite(pts).all(1)
    assert finite.all()
    tri_d, pts_d = _cuda(tri), _cuda(pts)
    w = dsdf.mesh_winding(tri_d, pts_d).cpu().numpy().astype(np.float64)
    walk = dsdf.MeshBvh(tri_d).winding(pts_d, beta=float('inf')).cpu().numpy().astype(np.float64)
    e64, ewalk = np.abs(w - WO.winding(pts, tri))[finite].max(), np.abs(w - walk)[finite].max()
    print(f'T = {T}: max |w - w_fp64| = {e64:.3e}, |w - walk(inf)| = {ewalk:.3e}')
    assert e64 <= WO.GATE and ewalk <= WO.GATE
