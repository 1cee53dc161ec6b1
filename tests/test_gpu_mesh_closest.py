"""GPU checks of the closest-point queries (include/dsdf.h: dsdf_mesh_closest, dsdf_mesh_bvh_closest) and of what is built on them:
dsdf.MeshBvh.closest returns BITWISE what the brute-force dsdf.mesh_closest returns and both match the fp64 reference
(tests/mesh_closest_oracle.py); dsdf.sample_surface, dsdf.mesh_distance, mesh_to_sdf.refine(distance='closest') and mesh_distance.py.

GATE.  mesh_closest_oracle.GATE = 4 x the maximum fp32 error measured on the HOST build of the same statements (7.577e-07 -> 3.031e-06,
tests/test_mesh_closest_host.py); the device runs the same uncontracted statements and gets the same gate.  Measured on the MI355X over
the same inputs: max |dist - dist_fp64| = 7.577e-07 (ico320), the host's figure to the digit; 5.703e-07 on the 1280-triangle mesh that
only the device sees.  A point sampled ON a mesh is rounded to fp32 (coordinates below 0.5: at most 2^-26 per axis, sqrt(3) 2^-26 = 2.6e-08
in all), which is added where a sampled point is compared with its own surface (SELF_GATE = 3.057e-06); measured: Hausdorff distance of
icosphere(0.30, 3) to itself 1.650e-08, of the surface extracted from a .vol to its own mesh through mesh_distance.py 3.211e-07."""
import ctypes as C
import functools
import json
import math

import numpy as np
import pytest
import torch

import iso_cases as I
import mesh_closest_oracle as O
import mesh_oracle as M

pytestmark = pytest.mark.gpu

GATE = O.GATE
SELF_GATE = GATE + math.sqrt(3.0) * 2.0 ** -26
N_SAMPLES = 4000                    # per mesh in the mesh_distance tests: the fp64 reference is every point against every triangle


@pytest.fixture(scope='module')
def dsdf(built):
    import dsdf as m
    m.load()
    assert torch.cuda.is_available()
    return m


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ico(radius, subdiv, centre=(0.0, 0.0, 0.0)):
    v, f = M.icosphere(radius, subdiv, centre=centre)
    return np.ascontiguousarray(v[f], np.float32)


GPU_MESHES = dict(O.MESHES, ico1280=_ico(0.3, 3, (0.05, -0.02, 0.01)))         # more than one tile of the brute-force kernel, a deeper tree


@functools.lru_cache(maxsize=None)
def points_and_reference(name):
    tri = GPU_MESHES[name]
    pts = O.all_points(tri, len(name), n_random=2000 if name == 'ico1280' else 20000)
    return pts, O.closest(pts, tri)


def _query(dsdf, tri_d, bvh, pts_d, **kw):
    a = bvh.closest(pts_d, return_prim=True, return_point=True, return_bary=True, **kw)
    b = dsdf.mesh_closest(tri_d, pts_d, return_prim=True, return_point=True, return_bary=True, **kw)
    return a, b


def _same_bits(a, b):
    return all(x.shape == y.shape and x.dtype == y.dtype and torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


# ---- 1, 2. the two kernels against each other and against the reference ------------------------------------------------------------------
@pytest.mark.parametrize('name', list(GPU_MESHES))
def test_bvh_is_bitwise_brute_force_and_matches_fp64(dsdf, name):
    tri = GPU_MESHES[name]
    pts, (d64, _) = points_and_reference(name)
    tri_d, pts_d = _cuda(tri), _cuda(pts)
    bvh = dsdf.MeshBvh(tri_d)
    for n in (pts.shape[0], 257, 1, 0):
        a, b = _query(dsdf, tri_d, bvh, pts_d[:n])
        assert _same_bits(a, b), (name, n)
        assert a[0].shape == (n,) and a[1].dtype == torch.int32 and a[2].shape == (n, 3) and a[3].shape == (n, 2)
        if n == pts.shape[0]:
            full = a
        else:
            assert _same_bits(a, [t[:n] for t in full]), (name, n)
    assert torch.equal(bvh.closest(pts_d), full[0]) and torch.equal(dsdf.mesh_closest(tri_d, pts_d), full[0])       # (the optional outputs are optional)
    dist, prim, point, bary = (t.cpu().numpy() for t in full)
    assert (prim >= 0).all() and (prim < tri.shape[0]).all()
    err = np.abs(dist.astype(np.float64) - d64).max()
    own = np.abs(O.dist_to_triangle(pts, tri[prim]) - d64).max()              # a different winner at a tie is as near
    print(f'{name}: device max |dist - dist_fp64| = {err:.3e}, |dist64(x, tri[prim]) - oracle| = {own:.3e}')
    assert err <= GATE and own <= GATE
    t = tri[prim].astype(np.float64)
    u, v = bary[:, :1].astype(np.float64), bary[:, 1:].astype(np.float64)
    assert np.abs(t[:, 0] + u * (t[:, 1] - t[:, 0]) + v * (t[:, 2] - t[:, 0]) - point).max() <= 1e-6
    assert (bary >= 0).all() and (bary.sum(1) <= 1 + 1e-6).all()


# ---- 3. max_dist, argument validation --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['ico320', 'T5', 'degenerate'])
def test_max_dist(dsdf, name):
    tri = GPU_MESHES[name]
    pts, _ = points_and_reference(name)
    tri_d, pts_d = _cuda(tri), _cuda(pts)
    bvh = dsdf.MeshBvh(tri_d)
    ref = _query(dsdf, tri_d, bvh, pts_d)[1]
    for max_dist in (0.0, 0.05, float(ref[0].median()), 1e30):
        keep = ref[0] <= max_dist
        a, b = _query(dsdf, tri_d, bvh, pts_d, max_dist=max_dist)
        assert _same_bits(a, b), (name, max_dist)
        assert torch.equal(a[1], torch.where(keep, ref[1], torch.full_like(ref[1], -1)))
        assert torch.equal(a[0], torch.where(keep, ref[0], torch.full_like(ref[0], float('inf'))))
        assert _same_bits([t[keep] for t in a], [t[keep] for t in ref])
        assert not a[2][~keep].any() and not a[3][~keep].any()
    verts = _cuda(O.query_points(tri, 0)['vertices'])                          # max_dist = 0 finds a point exactly on a vertex
    for d, p in (bvh.closest(verts, max_dist=0.0, return_prim=True), dsdf.mesh_closest(tri_d, verts, max_dist=0.0, return_prim=True)):
        assert bool((d == 0).all()) and bool((p >= 0).all())


def test_argument_validation(dsdf):
    lib = dsdf.load()
    one = C.c_void_p(16)            # never dereferenced: validation fails first
    inf = C.c_float(float('inf'))
    brute = lambda tri=one, T=4, pts=one, n=8, md=inf, out=one: lib.dsdf_mesh_closest(tri, T, pts, n, md, out, None, None, None, None)
    viabvh = lambda bvh=one, pts=one, n=8, md=inf, out=one: lib.dsdf_mesh_bvh_closest(bvh, pts, n, md, out, None, None, None, None)
    for call, name, bad in ((brute, b'dsdf_mesh_closest', [dict(tri=None), dict(T=0), dict(pts=None), dict(out=None), dict(n=-1),
                                                          dict(md=C.c_float(-1.0)), dict(md=C.c_float(float('nan')))]),
                            (viabvh, b'dsdf_mesh_bvh_closest', [dict(bvh=None), dict(pts=None), dict(out=None), dict(n=-1),
                                                                dict(md=C.c_float(-1.0)), dict(md=C.c_float(float('nan')))])):
        for kw in bad:
            assert call(**kw) == -1 and lib.dsdf_last_error().startswith(name), (name, kw, lib.dsdf_last_error())
    assert lib.dsdf_mesh_closest(None, 0, None, 0, inf, None, None, None, None, None) == 0           # n = 0: no launch, no pointers
    assert lib.dsdf_mesh_bvh_closest(None, None, 0, inf, None, None, None, None, None) == 0
    tri_d = _cuda(GPU_MESHES['box12'])
    bvh = dsdf.MeshBvh(tri_d)
    pts = torch.zeros(5, 3)
    for fn in (bvh.closest, lambda p, **kw: dsdf.mesh_closest(tri_d, p, **kw)):
        with pytest.raises(dsdf.DsdfError, match='no CPU path'):
            fn(pts)
        with pytest.raises(dsdf.DsdfError, match=r'\(N,3\)'):
            fn(pts.cuda().reshape(-1))
        with pytest.raises(dsdf.DsdfError, match='float32'):
            fn(pts.cuda().double())
        with pytest.raises(dsdf.DsdfError, match='dsdf_mesh'):
            fn(pts.cuda(), max_dist=-1.0)
    with pytest.raises(dsdf.DsdfError, match='no CPU path'):
        dsdf.mesh_closest(tri_d.cpu(), pts.cuda())
    with pytest.raises(dsdf.DsdfError, match='no CPU path'):
        dsdf.sample_surface(tri_d.cpu(), 10)


# ---- 4. sample_surface -----------------------------------------------------------------------------------------------------------------
def test_sample_surface(dsdf):
    tri = GPU_MESHES['box12']
    n = 120_000
    pts, prim, bary = dsdf.sample_surface(_cuda(tri), n, seed=3)
    assert pts.shape == (n, 3) and pts.dtype == torch.float32 and prim.shape == (n,) and bary.shape == (n, 2)
    again = dsdf.sample_surface(_cuda(tri), n, seed=3)
    assert all(torch.equal(x, y) for x, y in zip((pts, prim, bary), again))
    assert not torch.equal(pts, dsdf.sample_surface(_cuda(tri), n, seed=4)[0])
    p, k, uv = pts.cpu().numpy(), prim.cpu().numpy(), bary.cpu().numpy().astype(np.float64)
    on = O.dist_to_triangle(p, tri[k]).max()
    print(f'sample_surface: max distance of a sampled point to its own triangle {on:.3e}')
    assert on <= SELF_GATE
    t = tri[k].astype(np.float64)
    assert np.abs(t[:, 0] + uv[:, :1] * (t[:, 1] - t[:, 0]) + uv[:, 1:] * (t[:, 2] - t[:, 0]) - p).max() <= 1e-6
    assert (uv >= 0).all() and (uv.sum(1) <= 1 + 1e-6).all()
    t64 = tri.astype(np.float64)
    area = 0.5 * np.linalg.norm(np.cross(t64[:, 1] - t64[:, 0], t64[:, 2] - t64[:, 0]), axis=1)
    share = area / area.sum()
    assert len(np.unique(np.round(area, 9))) == 3                             # three distinct areas
    counts = np.bincount(k, minlength=len(tri))
    sigma = np.sqrt(n * share * (1 - share))
    assert (np.abs(counts - n * share) <= 5 * sigma).all(), (counts, n * share)
    # uniform INSIDE the triangles too: the mean of the samples of a triangle is its centroid (u, v each 1/3 +- 5 sigma, var 1/18)
    for j in range(len(tri)):
        assert np.abs(uv[k == j].mean(0) - 1 / 3).max() <= 5 * math.sqrt(1 / 18 / counts[j])
    # a triangle without area receives none; a mesh without area is an error
    a, b = np.float32([-0.25, 0.125, 0.5]), np.float32([0.75, -0.375, 0.0])
    flat = np.stack([np.stack([a, (a + b) / 2, b]), np.stack([a, a, a]), np.stack([a, a, b])]).astype(np.float32)      # EXACTLY collinear, a point, a segment
    deg = np.concatenate([tri[:6], flat, tri[6:]])
    kd = dsdf.sample_surface(_cuda(deg), 50_000, seed=0)[1].cpu().numpy()
    assert not np.isin(kd, (6, 7, 8)).any() and kd.min() >= 0 and kd.max() < len(deg)
    lead = np.concatenate([flat, tri[:6], flat])                              # zero area first and last
    kl = dsdf.sample_surface(_cuda(lead), 50_000, seed=0)[1].cpu().numpy()
    assert kl.min() >= 3 and kl.max() <= 8
    with pytest.raises(dsdf.DsdfError, match='no surface'):
        dsdf.sample_surface(_cuda(flat), 10)


# ---- 5. mesh_distance ------------------------------------------------------------------------------------------------------------------
def _recompute(res, tri_a, tri_b, threshold):
    """Every metric in fp64 from the returned sample points."""
    d1 = O.closest(res['points_a'].cpu().numpy(), tri_b)[0]
    d2 = O.closest(res['points_b'].cpu().numpy(), tri_a)[0]
    out = {'a_to_b_mean': d1.mean(), 'b_to_a_mean': d2.mean(), 'a_to_b_max': d1.max(), 'b_to_a_max': d2.max(),
           'chamfer_l1': (d1.mean() + d2.mean()) / 2, 'chamfer_l2': (d1 * d1).mean() + (d2 * d2).mean(), 'hausdorff': max(d1.max(), d2.max())}
    if threshold is not None:
        p, r = (d1 <= threshold).mean(), (d2 <= threshold).mean()
        out.update(precision=p, recall=r, fscore=2 * p * r / (p + r) if p + r > 0 else 0.0)
    return out, d1, d2


def test_mesh_distance_to_itself(dsdf):
    tri = _ico(0.30, 3)
    res = dsdf.mesh_distance(_cuda(tri), dsdf.MeshBvh(_cuda(tri)), n=N_SAMPLES, threshold=1e-5)
    print(f"mesh_distance of a mesh to itself: hausdorff {res['hausdorff']:.3e}, chamfer_l1 {res['chamfer_l1']:.3e}")
    assert 0 <= res['hausdorff'] <= SELF_GATE and res['chamfer_l1'] <= SELF_GATE
    assert res['precision'] == res['recall'] == res['fscore'] == 1.0
    assert res['points_a'].shape == (N_SAMPLES, 3) and res['dist_b_to_a'].shape == (N_SAMPLES,)
    assert not torch.equal(res['points_a'], res['points_b'])


@pytest.mark.parametrize('pair', ['radius', 'translated'])
def test_mesh_distance_matches_fp64(dsdf, pair):
    tri_a = _ico(0.30, 3)
    tri_b = _ico(0.32, 3) if pair == 'radius' else _ico(0.30, 3, (0.05, 0.0, 0.0))
    res = dsdf.mesh_distance(_cuda(tri_a), _cuda(tri_b), n=N_SAMPLES, seed=2, threshold=0.03)
    want, d1, d2 = _recompute(res, tri_a, tri_b, 0.03)
    assert set(want) | {'points_a', 'points_b', 'dist_a_to_b', 'dist_b_to_a'} == set(res)
    assert np.abs(res['dist_a_to_b'].cpu().numpy() - d1).max() <= GATE and np.abs(res['dist_b_to_a'].cpu().numpy() - d2).max() <= GATE
    for k, v in want.items():
        print(f'{pair}: {k} = {res[k]:.9g} (fp64 {v:.9g})')
        if k in ('precision', 'recall', 'fscore'):
            assert res[k] == v, k
        else:
            assert abs(res[k] - v) <= GATE, k
    if pair == 'radius':
        assert 0.015 < res['chamfer_l1'] < 0.025                              # a bracket around the 0.02 of two spheres, not a precision claim
        assert res['fscore'] == 1.0
    else:
        assert 0.0 < res['precision'] < 1.0 and 0.0 < res['fscore'] < 1.0      # the threshold cuts through the distribution
    none = dsdf.mesh_distance(_cuda(tri_a), _cuda(tri_b), n=100, seed=2)
    assert 'precision' not in none and 'fscore' not in none
    far = dsdf.mesh_distance(_cuda(tri_a), _cuda(tri_b + np.float32(2.0)), n=100, threshold=0.03)
    assert far['precision'] == far['recall'] == far['fscore'] == 0.0


# ---- 6. refine / create_sdf with distance='closest' ------------------------------------------------------------------------------------
def test_refine_with_closest_point_distance(dsdf):
    import mesh_to_sdf
    import redistancing
    res = 32
    tri = _ico(0.3, 2)
    tri_d = _cuda(tri).reshape(-1, 3, 3)
    values, origins = mesh_to_sdf.occupancy(tri_d, res)
    grid = redistancing.redistance(values)
    rays = mesh_to_sdf.refine(tri_d, grid, origins, res)
    assert torch.equal(mesh_to_sdf.refine(tri_d, grid, origins, res, distance='rays').view(torch.int32), rays.view(torch.int32))     # (c)
    close = mesh_to_sdf.refine(tri_d, grid, origins, res, distance='closest')
    assert torch.equal(mesh_to_sdf.refine(tri_d, grid, origins, res, distance='closest', accel='bvh').view(torch.int32), close.view(torch.int32))
    with pytest.raises(ValueError, match='distance'):                                                                                # (d)
        mesh_to_sdf.refine(tri_d, grid, origins, res, distance='nope')
    with pytest.raises(ValueError, match='distance'):
        mesh_to_sdf.create_sdf(tri_d, res, distance='nope')
    g, r, c = (t.reshape(-1).cpu().numpy().astype(np.float64) for t in (grid, rays, close))
    near = np.abs(g) < 1.0 / res
    assert near.sum() > 500
    assert np.array_equal(c[~near], g[~near])                                 # only the near-surface voxels change
    d64 = O.closest(origins.cpu().numpy()[near], tri)[0]
    assert np.abs(c[near] - np.where(g[near] < 0, -d64, d64)).max() <= GATE                                                          # (a)
    assert (np.abs(c[near]) <= np.abs(r[near]) + GATE).all()                                                                          # (b)
    share = (np.abs(c[near]) < np.abs(r[near])).mean()
    print(f'refine: {near.sum()} near-surface voxels, closest < rays at {100 * share:.1f} %, largest excess of the ray minimum '
          f'{(np.abs(r[near]) - np.abs(c[near])).max():.3e}')
    assert share > 0.5
    full = mesh_to_sdf.create_sdf(tri_d, res, distance='closest')
    ref = mesh_to_sdf.create_sdf(tri_d, res)
    assert full.shape == (res, res, res) and bool(torch.isfinite(full).all())
    assert float((full - ref).abs().max()) < 1.0 / res and bool(((full < 0) == (ref < 0)).all())


# ---- 7. mesh_distance.py ---------------------------------------------------------------------------------------------------------------
def test_cli_on_two_meshes(dsdf, tmp_path, capsys):
    import mesh_distance
    import mesh_to_sdf
    fa, fb, out = str(tmp_path / 'a.ply'), str(tmp_path / 'b.ply'), str(tmp_path / 'm.json')
    mesh_to_sdf.save_ply(fa, *M.icosphere(0.30, 2))
    mesh_to_sdf.save_ply(fb, *M.icosphere(0.32, 2))
    assert mesh_distance.main([fa, fb, '--samples', str(N_SAMPLES), '--seed', '5', '--threshold', '0.03', '--json', out]) == 0
    got = json.load(open(out))
    want = dsdf.mesh_distance(_cuda(mesh_to_sdf.load_mesh(fa)), _cuda(mesh_to_sdf.load_mesh(fb)), n=N_SAMPLES, seed=5, threshold=0.03)
    assert list(got) == list(mesh_distance.METRICS)
    assert all(got[k] == want[k] for k in mesh_distance.METRICS)
    printed = dict(line.split(': ') for line in capsys.readouterr().out.strip().splitlines())
    assert list(printed) == list(mesh_distance.METRICS) and all(abs(float(printed[k]) - got[k]) <= 1e-8 for k in got)
    assert 0.015 < got['chamfer_l1'] < 0.025
    assert mesh_distance.main([fa, fb, '--samples', '100']) == 0              # no threshold, no file


def test_cli_shifts_an_extracted_surface_into_the_scene_frame(dsdf, tmp_path):
    """A .vol against the mesh of its own surface, moved to where scene meshes live ([-0.5, 0.5]^3): zero distance only if mesh_distance.py
    applies the same shift to what it extracts (an unshifted surface is 0.5 off on every axis)."""
    import mesh_distance
    import mesh_to_sdf
    import util
    data = torch.from_numpy(I.grid('sphere16')).float()
    util.write_vol(str(tmp_path / 'sdf.vol'), data)
    v, f = dsdf.extract_mesh(dsdf.SdfGrid(data.cuda().contiguous()), resolution=12, normals=False)
    mesh_to_sdf.save_ply(str(tmp_path / 'own.ply'), v - 0.5, f)
    out = str(tmp_path / 'm.json')
    assert mesh_distance.main([str(tmp_path / 'sdf.vol'), str(tmp_path / 'own.ply'), '--res', '12', '--samples', str(N_SAMPLES), '--json', out]) == 0
    got = json.load(open(out))
    print(f"mesh_distance.py, a .vol against its own surface: hausdorff {got['hausdorff']:.3e}")
    assert got['hausdorff'] <= SELF_GATE
    mesh_to_sdf.save_ply(str(tmp_path / 'unshifted.ply'), v, f)
    assert mesh_distance.main([str(tmp_path / 'sdf.vol'), str(tmp_path / 'unshifted.ply'), '--res', '12', '--samples', '500', '--json', out]) == 0
    assert json.load(open(out))['hausdorff'] > 0.5
