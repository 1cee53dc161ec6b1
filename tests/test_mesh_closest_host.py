"""CPU check of the closest-point queries of the mesh BVH (csrc/dsdf_bvh.h: tri_closest, box_dist2, bvh_closest) through their stand-alone
host build (tests/harness/dsdf_closest_host.cpp): the stackless descent must return BITWISE the distance, triangle index, point and
barycentrics of the loop over all triangles, and both must agree with the fp64 reference (tests/mesh_closest_oracle.py).

GATE.  The fp32 error of this arithmetic was measured, not guessed: max |dist_fp32 - dist_fp64| over every mesh and point set below
(host build, query points in [-1, 1]^3 and up to 10 extents = 6 units away) is 7.577e-07 (on the far points, where one ulp of the
distance is 4.8e-07; 1.9e-07 on the points in [-1, 1]^3); the gate is 4 x that, 3.031e-06 (the factor covers other random draws, not
other arithmetic; mesh_closest_oracle.GATE, shared with the GPU tests).  `PYTHONPATH=oracle:tests python tests/test_mesh_closest_host.py`
prints the measurement."""
import ctypes as C

import numpy as np
import pytest

import mesh_closest_oracle as O
from host_build import ptr as _p, run_case, sanitized_program, shared_lib
from mesh_bvh_cases import morton_order, n_leaves

GATE = O.GATE


def load_host():
    return shared_lib('dsdf_closest_host.cpp', long_returning=['closest_host_size'])


@pytest.fixture(scope='module')
def host():
    return load_host()


def build(host, tri, order):
    T = tri.shape[0]
    assert host.closest_host_size(T) == 64 * n_leaves(T)
    buf = np.full(64 * n_leaves(T), np.nan, np.float32)
    host.closest_host_build(_p(tri), _p(order), T, _p(buf))
    return buf


def query(host, tri, pts, max_dist=np.inf, buf=None):
    """(dist, prim, point, bary) of the loop over all triangles (buf None) or of the traversal of `buf`."""
    n = pts.shape[0]
    dist = np.zeros(n, np.float32); prim = np.zeros(n, np.int32); point = np.zeros((n, 3), np.float32); bary = np.zeros((n, 2), np.float32)
    if buf is None:
        host.closest_host_brute(_p(tri), int(tri.shape[0]), _p(pts), C.c_long(n), C.c_float(max_dist), _p(dist), _p(prim), _p(point), _p(bary))
    else:
        host.closest_host_bvh(_p(buf), _p(pts), C.c_long(n), C.c_float(max_dist), _p(dist), _p(prim), _p(point), _p(bary))
    return dist, prim, point, bary


def same_bits(a, b):
    return all(np.array_equal(x.view(np.int32), y.view(np.int32)) for x, y in zip(a, b))


_cache = {}


def case(host, name):
    """Points, brute-force result and fp64 reference of one mesh, computed once."""
    if name not in _cache:
        tri = O.MESHES[name]
        pts = O.all_points(tri, len(name))
        _cache[name] = (tri, pts, query(host, tri, pts), O.closest(pts, tri))
    return _cache[name]


@pytest.mark.parametrize('name', list(O.MESHES))
def test_traversal_is_bitwise_brute_force(host, name):
    tri, pts, ref, _ = case(host, name)
    for order in (None, morton_order(tri), np.arange(tri.shape[0], dtype=np.int32)):      # (None: the harness's own Morton order)
        got = query(host, tri, pts, buf=build(host, tri, order))
        assert same_bits(got, ref), name
    assert (ref[1] >= 0).all() and np.isfinite(ref[0]).all()


@pytest.mark.parametrize('name', list(O.MESHES))
def test_against_fp64_oracle(host, name):
    tri, pts, (dist, prim, point, bary), (d64, _) = case(host, name)
    err = np.abs(dist.astype(np.float64) - d64).max()
    own = np.abs(O.dist_to_triangle(pts, tri[prim]) - d64).max()          # a different winner at a tie is as near
    print(f'{name}: max |dist_fp32 - dist_fp64| = {err:.3e}, |dist64(x, tri[prim]) - oracle| = {own:.3e}')
    assert err <= GATE and own <= GATE
    t = tri[prim].astype(np.float64)
    u, v = bary[:, :1].astype(np.float64), bary[:, 1:].astype(np.float64)
    assert np.abs(t[:, 0] + u * (t[:, 1] - t[:, 0]) + v * (t[:, 2] - t[:, 0]) - point).max() <= 1e-6
    assert (bary >= 0).all() and (bary.sum(1) <= 1 + 1e-6).all()
    assert np.abs(np.linalg.norm(pts.astype(np.float64) - point, axis=1) - d64).max() <= GATE + 1e-6


def test_oracle_against_sampling():
    """The reference itself: never above the minimum over a dense sampling of the triangle, and within the sampling step of it."""
    rng = np.random.default_rng(3)
    tris = np.concatenate([O.MESHES['ico80'][:20], O.MESHES['degenerate'][4:10], rng.uniform(-0.5, 0.5, (30, 3, 3))]).astype(np.float64)
    for k, t in enumerate(tris):
        for x in rng.uniform(-1, 1, (4, 3)):
            d, s = float(O.dist_to_triangle(x, t)), O.sampled_distance(x, t)
            step = max(np.linalg.norm(t[1] - t[0]), np.linalg.norm(t[2] - t[0])) / 300
            assert d <= s + 1e-12 and s - d <= 2 * step, (k, d, s)


def test_degenerate_triangles(host):
    """Collinear corners: the distance to the longest segment; three equal corners: to the point; finite for every finite input."""
    rng = np.random.default_rng(5)
    a, b = np.float32([-0.25, 0.125, 0.5]), np.float32([0.75, -0.375, 0.0])
    mid = ((a + b) / 2).astype(np.float32)                                  # exact in fp32: three collinear corners
    tris = np.stack([np.stack([a, mid, b]), np.stack([a, b, mid]), np.stack([mid, a, b]), np.stack([a, a, b]), np.stack([a, b, b]),
                     np.stack([b, a, b]), np.stack([a, a, a]), np.zeros((3, 3), np.float32), np.full((3, 3), 3e38, np.float32),
                     np.stack([a, a + np.float32(1e-30), b])]).astype(np.float32)
    pts = rng.uniform(-1, 1, (400, 3)).astype(np.float32)
    for k, t in enumerate(tris):
        tt = np.ascontiguousarray(np.broadcast_to(t, (len(pts), 3, 3)))
        out = np.zeros((len(pts), 3), np.float32)
        host.closest_host_tri(_p(tt), _p(pts), C.c_long(len(pts)), _p(out))
        if k == 8:
            assert not np.isnan(out).any()                                  # (the squared distance overflows; nothing is NaN)
            continue
        assert np.isfinite(out).all(), k
        want = O.dist_to_triangle(pts, t[None])
        seg = O._segment(pts.astype(np.float64), a.astype(np.float64), (b if k < 6 or k == 9 else a).astype(np.float64))
        if k != 7:
            assert np.abs(want - seg).max() <= 1e-12, k
        assert np.abs(np.sqrt(out[:, 0].astype(np.float64)) - want).max() <= GATE, k
        assert (out[:, 1:] >= 0).all() and (out[:, 1] + out[:, 2] <= 1 + 1e-6).all()


@pytest.mark.parametrize('name', ['ico320', 'T5', 'degenerate'])
def test_max_dist(host, name):
    tri, pts, ref, _ = case(host, name)
    buf = build(host, tri, morton_order(tri))
    for max_dist in (0.0, 0.05, float(np.median(ref[0])), 1e30):
        lim = np.float32(max_dist)
        keep = ref[0] <= lim
        for got in (query(host, tri, pts, lim), query(host, tri, pts, lim, buf)):
            assert np.array_equal(got[1], np.where(keep, ref[1], -1))
            assert np.array_equal(got[0].view(np.int32), np.where(keep, ref[0], np.float32(np.inf)).view(np.int32))
            assert same_bits([g[keep] for g in got], [r[keep] for r in ref])
            assert not got[2][~keep].any() and not got[3][~keep].any()
    # max_dist = 0 finds a point that lies exactly on a vertex
    verts = O.query_points(tri, 0)['vertices']
    for got in (query(host, tri, verts, 0.0), query(host, tri, verts, 0.0, buf)):
        assert (got[0] == 0).all() and (got[1] >= 0).all()


def test_nan_point_terminates(host):
    tri = O.MESHES['ico320']
    pts = np.float32([[np.nan, 0, 0], [0, np.nan, 0.1], [np.nan] * 3, [0.1, 0.2, 0.3]])
    for buf in (None, build(host, tri, morton_order(tri))):
        dist, prim, point, bary = query(host, tri, pts, buf=buf)
        assert np.isinf(dist[:3]).all() and (prim[:3] == -1).all() and np.isfinite(dist[3]) and prim[3] >= 0


def test_standalone_program_under_sanitizers(tmp_path):
    """The stand-alone program (its own main, nothing loaded into Python) built with AddressSanitizer + UBSan: the same meshes and
    points, a NaN point among them, without and with a limit."""
    exe = sanitized_program('dsdf_closest_host.cpp')
    for name, tri in O.MESHES.items():
        pts = np.concatenate([O.all_points(tri, len(name), n_random=2000), np.float32([[np.nan, 0, 0]])])
        for max_dist in (np.inf, 0.3):
            fn = tmp_path / f'{name}.bin'
            with open(fn, 'wb') as fh:
                fh.write(np.asarray([tri.shape[0], pts.shape[0]], np.int32).tobytes() + np.float32(max_dist).tobytes())
                fh.write(tri.tobytes() + pts.tobytes())
            run_case(exe, fn)


def test_python_layer_checks_that_need_no_device(tmp_path):
    """The `distance` keyword of mesh_to_sdf and the command line of mesh_distance.py are refused / parsed before any device work."""
    import torch
    import mesh_distance
    import mesh_to_sdf
    tri, grid, origins = torch.zeros(1, 3, 3), torch.zeros(2, 2, 2), torch.zeros(8, 3)
    with pytest.raises(ValueError, match="distance must be 'rays' or 'closest'"):
        mesh_to_sdf.refine(tri, grid, origins, 2, distance='nope')
    with pytest.raises(ValueError, match="distance must be 'rays' or 'closest'"):
        mesh_to_sdf.create_sdf(tri, 2, distance='nope', device='cpu')
    with pytest.raises(ValueError, match='accel'):
        mesh_to_sdf.refine(tri, grid, origins, 2, distance='closest', accel='nope')
    a = mesh_distance.parse_args(['a.ply', 'b.vol'])
    assert (a.a, a.b, a.samples, a.seed, a.threshold, a.res, a.json) == ('a.ply', 'b.vol', 200_000, 0, None, None, None)
    a = mesh_distance.parse_args(['a.obj', 'b.ply', '--samples', '1000', '--seed', '3', '--threshold', '0.01', '--res', '64', '--json', 'm.json'])
    assert (a.samples, a.seed, a.threshold, a.res, a.json) == (1000, 3, 0.01, 64, 'm.json')
    for bad in (['a.stl', 'b.ply'], ['a.ply'], ['a.ply', 'b.ply', '--samples', '0']):
        with pytest.raises(SystemExit):
            mesh_distance.parse_args(bad)
    import dsdf
    for name in ('mesh_closest', 'mesh_distance', 'sample_surface'):
        assert callable(getattr(dsdf, name))
    assert callable(dsdf.MeshBvh.closest)
    with pytest.raises(dsdf.DsdfError, match='no CPU path'):
        dsdf.mesh_closest(tri, torch.zeros(4, 3))


if __name__ == '__main__':
    h = load_host()
    worst = 0.0
    for nm, tr in O.MESHES.items():
        pt = O.all_points(tr, len(nm))
        e = np.abs(query(h, tr, pt)[0].astype(np.float64) - O.closest(pt, tr)[0])
        near = np.abs(pt).max(1) <= 1
        print(f'{nm:12s} max |dist_fp32 - dist_fp64| = {e.max():.3e}  (points in [-1,1]^3: {e[near].max():.3e})')
        worst = max(worst, e.max())
    print(f'measured maximum {worst:.3e}; gate = 4 x = {4 * worst:.3e}')
