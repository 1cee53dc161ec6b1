"""GPU checks of the generalized winding number (include/dsdf.h: dsdf_mesh_winding, dsdf_mesh_bvh_moments, dsdf_mesh_bvh_winding) and of
what is built on it: dsdf.mesh_winding, dsdf.MeshBvh.winding / signed_distance, dsdf.mesh_signed_distance, mesh_to_sdf's sign='winding' and
its command line, against the fp64 reference in another formulation (tests/mesh_winding_oracle.py) and against the HOST build of the same
statements (tests/harness/dsdf_winding_host.cpp).

GATES.  mesh_winding_oracle.GATE = 4 x the maximum fp32 error of the exact sum measured on the HOST build (2.861e-06 -> 1.144e-05,
tests/test_mesh_winding_host.py); the device runs the same uncontracted statements with its own atan2f and gets the same gate.  The walk
at the default beta = 2 must stay within 0.1 of the fp64 exact sum (a condition, not a measurement: 0.4 is left to the threshold 0.5), and
must agree with the host build's walk within GATE: the far / near decisions are the same bits, only the roundings of the terms differ.
Measured on the MI355X over the same inputs: max |w - w_fp64| of dsdf.mesh_winding = 2.861e-06 (two_spheres), the host's figure to the
digit; 1.907e-06 on the 1280-triangle mesh that only the device sees; |walk(inf) - exact sum| <= 2.623e-06 (the same terms in another
order); |device walk(2) - host walk(2)| <= 3.576e-07; |walk(2) - w_fp64| <= 2.694e-02 (T4; 2.113e-02 on ico320, 1.684e-02 on ico1280)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import mesh_closest_oracle as CO
import mesh_oracle as M
import mesh_winding_oracle as O
from mesh_bvh_cases import morton_order
from test_mesh_winding_host import build as host_build, load_host, walk as host_walk

pytestmark = pytest.mark.gpu

GATE = O.GATE
CENTRE = (0.05, -0.02, 0.01)
ICO1280 = O._ico(0.3, 3, CENTRE)                       # more than one LDS tile of the brute-force kernel, a deeper tree; no voxel centre on it
GPU_MESHES = dict(O.MESHES, ico1280=ICO1280)


@pytest.fixture(scope='module')
def dsdf(built):
    import dsdf as m
    m.load()
    assert torch.cuda.is_available()
    return m


@pytest.fixture(scope='module')
def host():
    return load_host()


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def points_and_reference(name):
    if name in O.MESHES:
        return O.points_and_reference(name)
    pts = O.all_points(GPU_MESHES[name], len(name), n_random=2000)
    return pts, O.winding(pts, GPU_MESHES[name])


# ---- 1 - 4. the two kernels against the reference, each other and the host build -----------------------------------------------------
@pytest.mark.parametrize('name', list(GPU_MESHES))
def test_winding_matches_fp64_and_host(dsdf, host, name):
    tri = GPU_MESHES[name]
    pts, w64 = points_and_reference(name)
    tri_d, pts_d = _cuda(tri), _cuda(pts)
    bvh = dsdf.MeshBvh(tri_d)
    for n in (pts.shape[0], 257, 1, 0):
        exact, walk_inf, walk_2 = dsdf.mesh_winding(tri_d, pts_d[:n]), bvh.winding(pts_d[:n], beta=float('inf')), bvh.winding(pts_d[:n])
        assert all(t.shape == (n,) and t.dtype == torch.float32 for t in (exact, walk_inf, walk_2))
        if n == pts.shape[0]:
            full = (exact, walk_inf, walk_2)
        else:
            assert all(torch.equal(a, b[:n]) for a, b in zip((exact, walk_inf, walk_2), full)), (name, n)
    assert torch.equal(bvh.winding(pts_d, beta=2.0), full[2]) and bvh.moments is not None
    exact, walk_inf, walk_2 = (t.cpu().numpy().astype(np.float64) for t in full)
    host_2 = host_walk(host, host_build(host, tri, bvh.order.cpu().numpy()), pts, 2.0).astype(np.float64)
    figures = (np.abs(exact - w64).max(), np.abs(walk_inf - exact).max(), np.abs(walk_2 - host_2).max(), np.abs(walk_2 - w64).max())
    print(f'{name}: device max |w - w_fp64| = {figures[0]:.3e}, |walk(inf) - w| = {figures[1]:.3e}, |walk(2) - host walk(2)| = {figures[2]:.3e}, '
          f'|walk(2) - w_fp64| = {figures[3]:.3e}')
    assert figures[0] <= GATE and figures[1] <= GATE and figures[2] <= GATE
    assert figures[3] <= O.TREE_GATE
    for beta in (3.0, 4.0):
        assert np.abs(bvh.winding(pts_d, beta=beta).cpu().numpy() - w64).max() <= O.TREE_GATE


# ---- 5. other builds of the tree ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['T5', 'ico20', 'two_spheres', 'ico1280'])
def test_caller_given_order_and_normals_give_the_same_results(dsdf, name):
    lib = dsdf.load()
    tri = GPU_MESHES[name]
    pts_d, tri_d = _cuda(points_and_reference(name)[0]), _cuda(tri)
    want = dsdf.MeshBvh(tri_d).winding(pts_d)
    assert torch.equal(dsdf.MeshBvh(tri_d, normals=_cuda(np.ones_like(tri))).winding(pts_d), want)
    # the C ABI with the caller's own Morton permutation (numpy; the class sorts the library's codes)
    T, n = tri.shape[0], pts_d.shape[0]
    order = _cuda(morton_order(tri))
    buf = torch.empty(int(lib.dsdf_mesh_bvh_size(T, 0)), dtype=torch.float32, device='cuda')
    mom = torch.full((int(lib.dsdf_mesh_bvh_moments_size(T)),), float('nan'), dtype=torch.float32, device='cuda')
    w = torch.empty(n, dtype=torch.float32, device='cuda')
    st = torch.cuda.current_stream().cuda_stream
    assert lib.dsdf_mesh_bvh_build(tri_d.data_ptr(), None, order.data_ptr(), T, buf.data_ptr(), st) == 0
    assert lib.dsdf_mesh_bvh_moments(buf.data_ptr(), T, mom.data_ptr(), st) == 0
    assert lib.dsdf_mesh_bvh_winding(buf.data_ptr(), mom.data_ptr(), pts_d.data_ptr(), n, C.c_float(2.0), w.data_ptr(), st) == 0
    assert torch.equal(w, want) and not bool(torch.isnan(mom).any())


# ---- 6. signed distance --------------------------------------------------------------------------------------------------------------------
def test_signed_distance(dsdf, monkeypatch):
    tri = ICO1280
    pts, w64 = points_and_reference('ico1280')
    d64 = CO.closest(pts, tri)[0]
    clear = d64 > 1e-3
    want = np.where(w64 > 0.5, -d64, d64)
    assert clear.mean() > 0.9 and (want[clear] < 0).sum() > 50
    tri_d, pts_d = _cuda(tri), _cuda(pts)
    bvh = dsdf.MeshBvh(tri_d)
    unsigned = bvh.closest(pts_d)
    results = [dsdf.mesh_signed_distance(tri_d, pts_d), dsdf.mesh_signed_distance(bvh, pts_d), bvh.signed_distance(pts_d),
               bvh.signed_distance(pts_d, beta=float('inf'))]
    monkeypatch.setattr(dsdf.renderer, 'BVH_MIN_TRIANGLES', 1000)             # a tensor above the threshold goes through a tree of its own
    results.append(dsdf.mesh_signed_distance(tri_d, pts_d))
    for sd in results:
        assert torch.equal(sd.abs(), unsigned)
        sd = sd.cpu().numpy()
        assert np.array_equal(sd[clear] < 0, want[clear] < 0)
        assert np.abs(sd[clear] - want[clear]).max() <= CO.GATE
    with pytest.raises(dsdf.DsdfError, match='beta'):
        bvh.signed_distance(pts_d, beta=0.5)
    with pytest.raises(dsdf.DsdfError, match='beta'):
        dsdf.mesh_signed_distance(tri_d, pts_d, beta=0.5)


# ---- 7 - 9. mesh_to_sdf ----------------------------------------------------------------------------------------------------------------
RES = 32


@functools.lru_cache(maxsize=None)
def _ray_oracle():
    return M.occupancy(ICO1280, RES)


def test_winding_occupancy_equals_ray_occupancy(dsdf):
    import mesh_to_sdf
    tri_d = _cuda(ICO1280)
    rays, origins = mesh_to_sdf.occupancy(tri_d, RES)
    again, _ = mesh_to_sdf.occupancy(tri_d, RES, sign='rays')
    assert torch.equal(rays.view(torch.int32), again.view(torch.int32))
    occ_ref, margin = _ray_oracle()                                            # 'rays' is what it was: the oracle's occupancy
    sure = margin > 1e-4
    assert sure.mean() > 0.95 and (rays.cpu().numpy() == occ_ref)[sure].all()
    for accel in ('brute', 'bvh', None):
        wind, o = mesh_to_sdf.occupancy(tri_d, RES, sign='winding', accel=accel)
        assert torch.equal(wind, rays) and torch.equal(o, origins), accel
    assert float(rays.min()) == -0.5 and float(rays.max()) == 0.5 and 1000 < int((rays < 0).sum()) < 6000


def test_create_sdf_with_winding_sign(dsdf):
    import mesh_to_sdf
    tri_d = _cuda(ICO1280)
    ref = mesh_to_sdf.create_sdf(tri_d, RES)
    assert torch.equal(mesh_to_sdf.create_sdf(tri_d, RES, sign='rays').view(torch.int32), ref.view(torch.int32))
    for kw in (dict(), dict(accel='bvh'), dict(accel='brute')):
        assert torch.equal(mesh_to_sdf.create_sdf(tri_d, RES, sign='winding', **kw), ref), kw
    close = mesh_to_sdf.create_sdf(tri_d, RES, distance='closest')
    assert torch.equal(mesh_to_sdf.create_sdf(tri_d, RES, sign='winding', distance='closest'), close)
    with pytest.raises(ValueError, match='sign'):
        mesh_to_sdf.create_sdf(tri_d, RES, sign='nope')


# ---- 10. a mesh with a hole ----------------------------------------------------------------------------------------------------------------
def test_hole_changes_the_occupancy_only_next_to_it(dsdf):
    """ico320 with one triangle removed against the intact mesh: the removed triangle subtends at most area / (d - rho)^2 at a point d
    away from its centroid, rho its circumradius -- at d >= 2 rho that is area / rho^2 <= 3 sqrt(3) / 4 = 1.3 sr (the largest triangle
    in a circle), 0.10 of 4 pi; with the 0.1 of the tree it stays below the 0.5 between the intact mesh's 0 or 1 and the threshold."""
    import mesh_to_sdf
    intact, holed = O.MESHES['ico320'], O.MESHES['ico320_hole']
    t = intact[O.HOLE].astype(np.float64)
    a, b, c = (np.linalg.norm(t[i] - t[j]) for i, j in ((0, 1), (1, 2), (2, 0)))
    area = 0.5 * np.linalg.norm(np.cross(t[1] - t[0], t[2] - t[0]))
    rho = a * b * c / (4 * area)
    far = (np.linalg.norm(M.voxel_centres(RES) - t.mean(0), axis=1) >= 2 * rho).reshape(RES, RES, RES)
    want, _ = mesh_to_sdf.occupancy(_cuda(intact), RES, sign='winding')
    assert torch.equal(want, mesh_to_sdf.occupancy(_cuda(intact), RES)[0])
    for accel in ('brute', 'bvh'):
        got, _ = mesh_to_sdf.occupancy(_cuda(holed), RES, sign='winding', accel=accel)
        assert (got.cpu().numpy() == want.cpu().numpy())[far].all(), accel
        assert 0 < (~far).sum() < 400


# ---- 11. the command line ---------------------------------------------------------------------------------------------------------------
def test_command_line(dsdf, tmp_path):
    import mesh_to_sdf
    import util
    fn, out = str(tmp_path / 'm.ply'), str(tmp_path / 'm.vol')
    mesh_to_sdf.save_ply(fn, *M.icosphere(0.3, 2, centre=CENTRE))
    for opts, kw in ((['--sign', 'winding'], dict(sign='winding')), (['--sign', 'winding', '--distance', 'closest'], dict(sign='winding', distance='closest')),
                     ([], dict())):
        assert mesh_to_sdf.main([fn, '-o', out, '--res', '24'] + opts) == 0
        assert torch.equal(util.read_vol(out, 'cuda'), mesh_to_sdf.create_sdf(fn, 24, **kw)), opts
    with pytest.raises(SystemExit) as e:
        mesh_to_sdf.main([fn, '-o', out, '--sign', 'nope'])
    assert e.value.code not in (0, None)


# ---- 12. argument validation ------------------------------------------------------------------------------------------------------------
def test_argument_validation(dsdf):
    lib = dsdf.load()
    one = C.c_void_p(16)            # never dereferenced: validation fails first
    two = C.c_float(2.0)
    brute = lambda tri=one, T=4, pts=one, n=8, out=one: lib.dsdf_mesh_winding(tri, T, pts, n, out, None)
    moments = lambda bvh=one, T=4, out=one: lib.dsdf_mesh_bvh_moments(bvh, T, out, None)
    walk = lambda bvh=one, mom=one, pts=one, n=8, beta=two, out=one: lib.dsdf_mesh_bvh_winding(bvh, mom, pts, n, beta, out, None)
    for call, name, bad in ((brute, b'dsdf_mesh_winding', [dict(tri=None), dict(T=0), dict(pts=None), dict(out=None), dict(n=-1)]),
                            (moments, b'dsdf_mesh_bvh_moments', [dict(bvh=None), dict(T=0), dict(out=None)]),
                            (walk, b'dsdf_mesh_bvh_winding', [dict(bvh=None), dict(mom=None), dict(pts=None), dict(out=None), dict(n=-1),
                                                              dict(beta=C.c_float(0.5)), dict(beta=C.c_float(-3.0)), dict(beta=C.c_float(float('nan')))])):
        for kw in bad:
            assert call(**kw) == -1 and lib.dsdf_last_error().startswith(name), (name, kw, lib.dsdf_last_error())
    assert lib.dsdf_mesh_winding(None, 0, None, 0, None, None) == 0            # n = 0: no launch, no pointers
    assert lib.dsdf_mesh_bvh_winding(None, None, None, 0, two, None, None) == 0
    assert lib.dsdf_mesh_bvh_moments_size(0) == 0 and lib.dsdf_mesh_bvh_moments_size(5) == 32 and lib.dsdf_mesh_bvh_moments_size(1280) == 16 * 512
    tri_d = _cuda(GPU_MESHES['box12'])
    bvh = dsdf.MeshBvh(tri_d)
    pts = torch.zeros(5, 3)
    for fn in (bvh.winding, lambda p, **kw: dsdf.mesh_winding(tri_d, p, **kw)):
        with pytest.raises(dsdf.DsdfError, match='no CPU path'):
            fn(pts)
        with pytest.raises(dsdf.DsdfError, match=r'\(N,3\)'):
            fn(pts.cuda().reshape(-1))
        with pytest.raises(dsdf.DsdfError, match='float32'):
            fn(pts.cuda().double())
    for beta in (0.5, 0.0, float('nan')):
        with pytest.raises(dsdf.DsdfError, match='beta'):
            bvh.winding(pts.cuda(), beta=beta)
    # the moments of another tree are refused (NaN), not read out of bounds
    other = dsdf.MeshBvh(_cuda(ICO1280))
    pts_d, w = pts.cuda(), torch.zeros(5, device='cuda')
    assert bool(torch.isfinite(bvh.winding(pts_d)).all()) and bvh.moments.numel() == 16 * 4 and other.buffer.numel() == 64 * 512
    assert lib.dsdf_mesh_bvh_winding(other.buffer.data_ptr(), bvh.moments.data_ptr(), pts_d.data_ptr(), 5, two, w.data_ptr(),
                                     torch.cuda.current_stream().cuda_stream) == 0
    assert bool(torch.isnan(w).all())
