"""CPU check of the generalized winding number (csrc/dsdf_winding.h: tri_solid_angle, the per-node moments, bvh_winding) through its
stand-alone host build (tests/harness/dsdf_winding_host.cpp) against the fp64 reference in another formulation
(tests/mesh_winding_oracle.py).

GATE.  The fp32 error of the exact sum was measured, not guessed: max |w_fp32 - w_fp64| of the host build over every mesh and point set of
the oracle module is mesh_winding_oracle.MEASURED_MAX_ERR = 2.861e-06 (two_spheres; 2.742e-06 on box12); the gate is 4 x that (the factor covers other random draws and the device's
atan2f, not other arithmetic; shared with the GPU tests).  The dipole approximation has a CONDITION instead: at every beta of the tests
the walk stays within 0.1 of the fp64 exact sum on every mesh, and the error at beta = 4 does not exceed the one at beta = 2 (beyond
the fp32 rounding of the sum itself, GATE -- on a tree of one leaf every beta gives the same exact sum).
`PYTHONPATH=oracle:tests python tests/test_mesh_winding_host.py` prints the measurements (profiles/mesh_winding.md holds them)."""
import ctypes as C

import numpy as np
import pytest

import mesh_closest_oracle as CO
import mesh_winding_oracle as O
from host_build import ptr as _p, run_case, sanitized_program, shared_lib
from mesh_bvh_cases import morton_order, n_leaves

GATE = O.GATE


def load_host():
    return shared_lib('dsdf_winding_host.cpp', long_returning=['winding_host_size', 'winding_host_moments_size'])


@pytest.fixture(scope='module')
def host():
    return load_host()


def build(host, tri, order):
    """(bvh buffer, moments buffer) of the host build; both start as NaN so that a float nobody wrote shows."""
    T = tri.shape[0]
    L = n_leaves(T)
    assert host.winding_host_size(T) == 64 * L and host.winding_host_moments_size(T) == 16 * L
    buf, mom = np.full(64 * L, np.nan, np.float32), np.full(16 * L, np.nan, np.float32)
    host.winding_host_build(_p(tri), _p(order), T, _p(buf), _p(mom))
    return buf, mom


def brute(host, tri, pts):
    w = np.zeros(pts.shape[0], np.float32)
    host.winding_host_brute(_p(tri), int(tri.shape[0]), _p(pts), C.c_long(pts.shape[0]), _p(w))
    return w


def walk(host, tree, pts, beta):
    w = np.zeros(pts.shape[0], np.float32)
    assert host.winding_host_bvh(_p(tree[0]), _p(tree[1]), _p(pts), C.c_long(pts.shape[0]), C.c_float(beta), _p(w)) == 0
    return w


_cache = {}


def case(host, name):
    """Points, exact host sum, Morton-ordered tree and fp64 reference of one mesh, computed once."""
    if name not in _cache:
        tri = O.MESHES[name]
        pts, w64 = O.points_and_reference(name)
        _cache[name] = (tri, pts, brute(host, tri, pts), build(host, tri, morton_order(tri)), w64)
    return _cache[name]


def test_oracle_against_analytic_values():
    """The reference itself: 1 inside and 0 outside a closed sphere; 0.5 at the centre of the flat cap of a half-icosphere -- the faces of
    an icosphere come in antipodal pairs, so the faces on one side of a plane through its centre subtend exactly half of the sphere there."""
    tri = O.MESHES['ico320']
    rng = np.random.default_rng(0)
    x = rng.uniform(-0.6, 0.6, (3000, 3))
    r = np.linalg.norm(x, axis=1)
    x = x[(r < 0.28) | (r > 0.31)]
    w = O.winding(x, tri)
    assert np.abs(w - (np.linalg.norm(x, axis=1) < 0.29)).max() <= 1e-12
    half = O.MESHES['half_ico']
    assert half.shape[0] == 160
    w0 = O.winding(np.zeros((1, 3)), half)[0]
    print(f'oracle: w at the centre of the half-icosphere = {w0:.12f}')
    assert abs(w0 - 0.5) <= 1e-6                                   # (the fp32 rounding of the vertices is all that breaks the symmetry)
    # the single terms, against the octant of a sphere: the triangle (1,0,0), (0,1,0), (0,0,1) seen from the origin is 4 pi / 8
    octant = np.float64([[1, 0, 0], [0, 1, 0], [0, 0, 1]])
    assert abs(O.solid_angle(np.zeros(3), octant) - np.pi / 2) <= 1e-14 and abs(O.solid_angle(np.zeros(3), octant[::-1]) + np.pi / 2) <= 1e-14


@pytest.mark.parametrize('name', list(O.MESHES))
def test_exact_sum_against_fp64(host, name):
    tri, pts, w, _, w64 = case(host, name)
    err = np.abs(w.astype(np.float64) - w64).max()
    print(f'{name}: max |w_fp32 - w_fp64| = {err:.3e}')
    assert err <= GATE


@pytest.mark.parametrize('name', list(O.MESHES))
def test_tree_against_fp64_and_exact_walk(host, name):
    tri, pts, w, tree, w64 = case(host, name)
    err = {}
    for beta in O.BETAS:
        err[beta] = np.abs(walk(host, tree, pts, beta).astype(np.float64) - w64).max()
        print(f'{name}: beta = {beta:g}: max |w_tree - w_fp64| = {err[beta]:.3e}')
        assert err[beta] <= O.TREE_GATE, (name, beta)
    assert err[4.0] <= err[2.0] + GATE, name
    for order in (None, morton_order(tri), np.arange(tri.shape[0], dtype=np.int32)):      # (None: the harness's own Morton order)
        exact = walk(host, build(host, tri, order), pts, np.inf)
        assert np.abs(exact.astype(np.float64) - w.astype(np.float64)).max() <= GATE, name
        assert np.abs(exact.astype(np.float64) - w64).max() <= GATE, name
    assert np.array_equal(walk(host, build(host, tri, None), pts, 2.0), walk(host, tree, pts, 2.0))


def _subtree_corners(buf, T, L, i):
    """The corners of the filled slots below heap node i, from the layout of include/dsdf.h."""
    lo, hi = i, i
    while lo < L - 1:
        lo, hi = 2 * lo + 1, 2 * hi + 2
    slots = buf[16 * L:64 * L].reshape(4 * L, 12)[4 * (lo - (L - 1)):4 * (hi - (L - 1)) + 4]
    return slots[slots.view(np.int32)[:, 9] >= 0][:, :9].reshape(-1, 3).astype(np.float64)


@pytest.mark.parametrize('name', list(O.MESHES))
def test_moments(host, name):
    tri = O.MESHES[name]
    T, L = tri.shape[0], n_leaves(tri.shape[0])
    for order in (morton_order(tri), np.arange(T, dtype=np.int32)):
        buf, mom = build(host, tri, order)
        assert not np.isnan(mom).any()
        assert mom[:8].view(np.int32)[0] == L and not mom[1:8].any()
        rec = mom[8:].reshape(2 * L - 1, 8).astype(np.float64)
        for i in range(2 * L - 1):
            pts = _subtree_corners(buf, T, L, i)
            N, c, r, A = rec[i, :3], rec[i, 3:6], rec[i, 6], rec[i, 7]
            if len(pts) == 0:
                assert r == -1.0, (name, i)                         # the marker of an empty subtree
                continue
            assert r >= 0 and A >= 0, (name, i)
            assert (np.linalg.norm(pts - c, axis=1) <= r).all(), (name, i)        # every corner, hence every point, of the subtree
            t = pts.reshape(-1, 3, 3)
            n = 0.5 * np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
            area = np.linalg.norm(n, axis=1).sum()
            tol = (np.log2(L) + 8) * 2.0 ** -23 * max(area, 1e-30)
            assert np.abs(N - n.sum(0)).max() <= tol and abs(A - area) <= tol, (name, i)
            if area > 1e-12:
                g = (np.linalg.norm(n, axis=1)[:, None] * t.mean(1)).sum(0) / area
                assert np.abs(c - g).max() <= 1e-5, (name, i)
        if name in O.CLOSED:                                        # a closed surface: the normals cancel
            area = rec[0, 7]
            assert np.abs(rec[0, :3]).max() <= (np.log2(L) + 8) * 2.0 ** -23 * area, name
    if name == 'ico20':
        assert L == 8 and (mom[8:].reshape(-1, 8)[7 + 5:15, 6] == -1).all()       # 5 leaves filled, 3 empty


@pytest.mark.parametrize('name', ['box12', 'ico320', 'two_spheres'])
def test_integer_winding_number(host, name):
    """round(w) is the analytic count -- how many of the convex parts hold the point -- at every point farther than 1e-3 from the surface."""
    tri, pts, w, tree, _ = case(host, name)
    count, sure = O.analytic_count(name, pts)
    assert sure.mean() > 0.9 and set(count[sure]) == ({0, 1, 2} if name == 'two_spheres' else {0, 1})
    assert np.array_equal(np.rint(w[sure]).astype(int), count[sure])
    assert np.array_equal(np.rint(walk(host, tree, pts, 2.0)[sure]).astype(int), count[sure])
    assert np.abs(w[sure] - count[sure]).max() <= GATE


@pytest.mark.parametrize('name', list(O.MESHES))
def test_points_on_the_surface_are_finite(host, name):
    tri, _, _, tree, _ = case(host, name)
    pts = O.surface_points(tri, 0)
    assert np.isfinite(brute(host, tri, pts)).all()
    for beta in (2.0, np.inf):
        assert np.isfinite(walk(host, tree, pts, beta)).all()


def test_degenerate_triangles_contribute_nothing(host):
    """Collinear corners, a segment and a point: 0 at every point off their line, to the rounding of the determinant."""
    rng = np.random.default_rng(5)
    a, b = np.float32([-0.25, 0.125, 0.5]), np.float32([0.75, -0.375, 0.0])
    mid = ((a + b) / 2).astype(np.float32)                                  # exact in fp32: three collinear corners
    tris = np.stack([np.stack([a, mid, b]), np.stack([a, b, mid]), np.stack([a, a, b]), np.stack([a, b, b]), np.stack([a, a, a]),
                     np.zeros((3, 3), np.float32)]).astype(np.float32)
    pts = rng.uniform(-1, 1, (400, 3)).astype(np.float32)
    off = CO._segment(pts.astype(np.float64), a.astype(np.float64), b.astype(np.float64)) > 0.05
    for k, t in enumerate(tris):
        tt = np.ascontiguousarray(np.broadcast_to(t, (len(pts), 3, 3)))
        out = np.full(len(pts), np.nan, np.float32)
        host.winding_host_tri(_p(tt), _p(pts), C.c_long(len(pts)), _p(out))
        assert np.isfinite(out).all() and np.abs(out[off]).max() <= 4 * np.pi * GATE, k


def test_beta_below_one_is_refused(host):
    tri = O.MESHES['box12']
    tree = build(host, tri, None)
    pts = np.zeros((3, 3), np.float32)
    w = np.zeros(3, np.float32)
    for beta in (0.5, 0.999, 0.0, -2.0, float('nan')):
        assert host.winding_host_bvh(_p(tree[0]), _p(tree[1]), _p(pts), C.c_long(3), C.c_float(beta), _p(w)) == -1, beta
    for beta in (1.0, 2.0, float('inf')):
        assert host.winding_host_bvh(_p(tree[0]), _p(tree[1]), _p(pts), C.c_long(3), C.c_float(beta), _p(w)) == 0, beta


def test_standalone_program_under_sanitizers(tmp_path):
    """The stand-alone program (its own main, nothing loaded into Python) built with AddressSanitizer + UBSan: the same meshes, their
    query points and the points on their surfaces, a NaN point among them, at beta = 2 and beta = 1."""
    exe = sanitized_program('dsdf_winding_host.cpp')
    for name, tri in O.MESHES.items():
        pts = np.concatenate([O.all_points(tri, len(name), n_random=2000), O.surface_points(tri, 0), np.float32([[np.nan, 0, 0]])])
        for beta in (2.0, 1.0):
            fn = tmp_path / f'{name}.bin'
            with open(fn, 'wb') as fh:
                fh.write(np.asarray([tri.shape[0], pts.shape[0]], np.int32).tobytes() + np.float32(beta).tobytes())
                fh.write(tri.tobytes() + pts.tobytes())
            run_case(exe, fn)


def test_python_layer_checks_that_need_no_device():
    """The `sign` keyword and the command line of mesh_to_sdf are refused / parsed before any device work."""
    import torch
    import dsdf
    import mesh_to_sdf
    tri = torch.zeros(1, 3, 3)
    with pytest.raises(ValueError, match="sign must be 'rays' or 'winding'"):
        mesh_to_sdf.occupancy(tri, 2, sign='nope')
    with pytest.raises(ValueError, match="sign must be 'rays' or 'winding'"):
        mesh_to_sdf.create_sdf(tri, 2, sign='nope', device='cpu')
    with pytest.raises(ValueError, match='accel'):
        mesh_to_sdf._winder(tri, 'nope')
    a = mesh_to_sdf.parse_args(['m.ply', '-o', 'out.vol'])
    assert (a.mesh, a.out, a.res, a.sign, a.distance) == ('m.ply', 'out.vol', 128, 'rays', 'rays')
    a = mesh_to_sdf.parse_args(['m.obj', '-o', 'o.vol', '--res', '64', '--sign', 'winding', '--distance', 'closest'])
    assert (a.res, a.sign, a.distance) == (64, 'winding', 'closest')
    for bad in (['m.ply'], ['m.ply', '-o', 'o.vol', '--sign', 'nope'], ['m.ply', '-o', 'o.vol', '--distance', 'nope'], ['m.ply', '-o', 'o.vol', '--res', '1']):
        with pytest.raises(SystemExit) as e:
            mesh_to_sdf.parse_args(bad)
        assert e.value.code != 0
    for name in ('mesh_winding', 'mesh_signed_distance'):
        assert callable(getattr(dsdf, name))
    assert callable(dsdf.MeshBvh.winding) and callable(dsdf.MeshBvh.signed_distance)
    assert mesh_to_sdf.BVH_MIN_TRIANGLES == dsdf.renderer.BVH_MIN_TRIANGLES == 4096
    with pytest.raises(dsdf.DsdfError, match='no CPU path'):
        dsdf.mesh_winding(tri, torch.zeros(4, 3))
    with pytest.raises(dsdf.DsdfError, match='no CPU path'):
        dsdf.mesh_signed_distance(tri, torch.zeros(4, 3))


if __name__ == '__main__':
    h = load_host()
    worst = 0.0
    for nm, tr in O.MESHES.items():
        pt, w64 = O.points_and_reference(nm)
        e = np.abs(brute(h, tr, pt).astype(np.float64) - w64).max()
        tree = build(h, tr, morton_order(tr))
        te = [np.abs(walk(h, tree, pt, b).astype(np.float64) - w64).max() for b in O.BETAS]
        print(f'{nm:12s} {tr.shape[0]:5d} triangles: max |w_fp32 - w_fp64| = {e:.3e}; tree at beta = 2, 3, 4: ' + ', '.join(f'{x:.3e}' for x in te))
        worst = max(worst, e)
    print(f'MEASURED_MAX_ERR = {worst:.3e}; gate = 4 x = {4 * worst:.3e}')
