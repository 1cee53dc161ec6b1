"""CPU check of the surface extraction (csrc/dsdf_iso.h) through its stand-alone host build (tests/harness/dsdf_iso_host.cpp), which
runs the per-node and per-vertex statements of the four kernels serially, against the numpy oracle of tests/iso_cases.py: topology
EQUAL to the oracle's on the same value buffer, vertices on the rendered surface to fp32 noise of the lookup, orientation, second-order
convergence; the mesh writers; the argument checks of the four entry points of the built library."""
import ctypes as C

import numpy as np
import pytest

import iso_cases as I
from host_build import compile as compile_host, ptr as _p, run_case, sanitized_program, shared_lib
from iso_cases import ON_EDGE_TOL, VERTEX_RESIDUAL_GATE, assert_same_topology


class Host:
    def __init__(self, lib):
        self.lib = lib
        self._meshes = {}

    def sample(self, data, n, sdf_p=None):
        d = np.ascontiguousarray(data, np.float32)
        rz, ry, rx = d.shape
        values = np.full(I.n_nodes(n), np.nan, np.float32)
        sp = None if sdf_p is None else np.asarray(sdf_p, np.float32)
        self.lib.iso_host_sample(_p(d), rx, ry, rz, _p(sp), *n, _p(values))
        return values

    def topology(self, values, n, iso=0.0):
        N = I.n_nodes(n)
        cross = np.full(N, 255, np.uint8); nv = np.full(N, -1, np.int32); nt = np.full(N, -1, np.int32)
        self.lib.iso_host_mark(_p(values), *n, C.c_float(iso), _p(cross), _p(nv), _p(nt))
        vo = (np.cumsum(nv) - nv).astype(np.int32); to = (np.cumsum(nt) - nt).astype(np.int32)          # the caller's exclusive scans
        ve = np.full(int(nv.sum()), -1, np.int32); faces = np.full((int(nt.sum()), 3), -1, np.int32)
        self.lib.iso_host_emit(_p(values), *n, C.c_float(iso), _p(cross), _p(vo), _p(to), _p(ve), _p(faces))
        return dict(cross=cross, n_vert=nv, n_tri=nt, vert_edge=ve, faces=faces)

    def refine(self, data, values, n, vert_edge, iso=0.0, steps=24, sdf_p=None):
        d = np.ascontiguousarray(data, np.float32)
        rz, ry, rx = d.shape
        V = len(vert_edge)
        pos = np.full((V, 3), np.nan, np.float32); nrm = np.full((V, 3), np.nan, np.float32)
        sp = None if sdf_p is None else np.asarray(sdf_p, np.float32)
        self.lib.iso_host_refine(_p(d), rx, ry, rz, _p(sp), _p(values), *n, C.c_float(iso), _p(vert_edge), C.c_long(V), steps, _p(pos), _p(nrm))
        return pos, nrm

    def mesh(self, name, n):
        """Sampling, topology and vertices of a grid case through the harness (computed once)."""
        key = (name, tuple(n))
        if key not in self._meshes:
            values = self.sample(I.grid(name), n)
            t = self.topology(values, n)
            pos, nrm = self.refine(I.grid(name), values, n, t['vert_edge'])
            self._meshes[key] = dict(t, values=values, positions=pos, normals=nrm)
        return self._meshes[key]


@pytest.fixture(scope='module')
def host():
    return Host(shared_lib('dsdf_iso_host.cpp'))


def test_case_table_against_the_geometric_rule(host):
    """The library's swap bit of every (tetrahedron, mixed case) is what the rule gives -- with the vertices in the middle of their
    edges and anywhere else on them: the orientation is a function of (tetrahedron, case) alone."""
    rng = np.random.default_rng(5)
    for tet in range(6):
        for mask in range(1, 15):
            for tri in I.case_triangles(mask):
                want = I.needs_swap(tet, mask, tri)
                assert bool(host.lib.iso_host_swap(tet, mask)) == want, (tet, mask)
                for _ in range(8):
                    s = {(p, q): rng.uniform(0.01, 0.99) for p in range(4) for q in range(p + 1, 4)}
                    assert I.needs_swap(tet, mask, tri, s) == want, (tet, mask, s)


def test_random_lattice_has_every_case():
    n, values = I.VALUE_LATTICES['random_5x4x3']
    seen = {(int(t), int(m)) for t, m in I.topology(values, n)['tet_case']}
    assert seen == {(t, m) for t in range(6) for m in range(1, 15)}
    n, values = I.VALUE_LATTICES['zeros_5x4x3']
    assert (values == 0).sum() > 20                                          # exact zeros: outside


@pytest.mark.parametrize('name', list(I.VALUE_LATTICES))
def test_topology_of_value_lattices(host, name):
    """(a) on lattices of values handed over as they are, (b) where no inside node touches the border."""
    n, values = I.VALUE_LATTICES[name]
    ref = I.topology(values, n)
    got = host.topology(values, n)
    assert_same_topology(got, ref, name)
    rep = I.manifold_report(got['faces'], len(got['vert_edge']))
    if not I.border_inside(values, n):
        assert rep['closed'], rep
    if name == 'one_inside_2x2x2':
        assert len(got['vert_edge']) == 14 and len(got['faces']) == 24 and rep['closed'] and rep['euler'] == 2
    if name == 'one_on_border_2x2x2':
        assert not rep['closed'] and len(got['faces']) > 0
    # another level on the same buffer: the comparison is strict, a value equal to iso is outside
    iso = float(values[len(values) // 2])
    assert_same_topology(host.topology(values, n, iso), I.topology(values, n, iso), (name, iso))


GRID_RUNS = [(name, n) for name, n in I.GRID_CASES.items()] + [('sphere16', (24, 24, 24)), ('sphere16', (17, 16, 15))]


@pytest.mark.parametrize('name,n', GRID_RUNS, ids=[f'{a}-{"x".join(map(str, b))}' for a, b in GRID_RUNS])
def test_grid_topology_and_vertices(host, name, n):
    """(a), (b), (c) on the grids, values from the harness's own sampling."""
    m = host.mesh(name, n)
    ref64 = I.oracle_values(I.grid(name), n)
    assert np.linalg.norm(m['values'] - ref64) / np.linalg.norm(ref64) < 1e-6
    assert_same_topology(m, I.topology(m['values'], n), (name, n))
    V, F = len(m['vert_edge']), len(m['faces'])
    rep = I.manifold_report(m['faces'], V)
    assert V > 500 and not I.border_inside(m['values'], n) and rep['closed'], rep
    if name == 'sphere16':
        assert rep['euler'] == 2
    # (c) on its edge, on the surface
    a, b, _ = I.edge_endpoints(m['vert_edge'], n)
    pos = m['positions'].astype(np.float64)
    d = b - a
    s = ((pos - a) * d).sum(1) / (d * d).sum(1)
    off = np.linalg.norm(pos - (a + np.clip(s, 0.0, 1.0)[:, None] * d), axis=1)
    assert off.max() <= ON_EDGE_TOL, off.max()
    res = np.abs(I.f64(I.grid(name), pos)).max()
    print(f'{name} {n}: {V} vertices, {F} faces, euler {rep["euler"]}, max |f64(vertex)| = {res:.3e} (gate {VERTEX_RESIDUAL_GATE:.3e})')
    assert res <= VERTEX_RESIDUAL_GATE, res
    # normals: unit length, the normalised fp64 gradient
    _, g = I.f64(I.grid(name), pos, 1)
    g /= np.linalg.norm(g, axis=1, keepdims=True)
    assert np.abs(np.linalg.norm(m['normals'], axis=1) - 1).max() < 1e-6
    assert np.linalg.norm(m['normals'] - g) / np.linalg.norm(g) < 1e-5


def test_sphere_faces_follow_the_gradient(host):
    """(d) no face normal of sphere16 opposes the mean gradient of its corners."""
    m = host.mesh('sphere16', (16, 16, 16))
    pos = m['positions'].astype(np.float64)
    tri = pos[m['faces']]
    fn = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    _, g = I.f64(I.grid('sphere16'), pos, 1)
    opposed = ((fn * g[m['faces']].mean(1)).sum(1) <= 0).sum()
    assert len(fn) == 2232 == len(I.oracle_mesh_of('sphere16', (16, 16, 16))['faces']) and opposed == 0, opposed


def test_second_order_convergence(host):
    """(e) max |f(face centroid)| on sphere16 shrinks by at least 2.5 x per halving of the cell (second order predicts 4 x; the fp64
    reference gives 1.63e-2, 3.40e-3, 9.17e-4)."""
    err = []
    for n in (8, 16, 32):
        m = host.mesh('sphere16', (n, n, n))
        cen = m['positions'].astype(np.float64)[m['faces']].mean(1)
        err.append(np.abs(I.f64(I.grid('sphere16'), cen)).max())
    print('max |f(centroid)| at n = 8, 16, 32:', err)
    assert err[0] / err[1] >= 2.5 and err[1] / err[2] >= 2.5, err


def test_frame_is_the_cubes_own(host):
    """`sdf.p` plays no part in the library calls, and neither does the transform of a world-space build (-DDSDF_XF=1)."""
    n = (16, 16, 16)
    m = host.mesh('sphere16', n)
    assert np.array_equal(host.sample(I.grid('sphere16'), n, sdf_p=(0.25, -0.5, 0.125)), m['values'])
    xf = Host(C.CDLL(compile_host('dsdf_iso_host.cpp', 'libdsdf_iso_host_xf.so', ['-shared', '-fPIC', '-DDSDF_XF=1'])))
    assert xf.lib.iso_host_xf() == 1 and host.lib.iso_host_xf() == 0
    c, s = np.cos(0.3), np.sin(0.3)
    to_local = np.array([[1.5 * c, -s, 0, 0.1], [s, 0.8 * c, 0, -0.2], [0, 0, 1.25, 0.05]], np.float32)
    xf.lib.iso_host_set_transform(_p(to_local))
    values = xf.sample(I.grid('sphere16'), n, sdf_p=(0.25, -0.5, 0.125))
    assert np.array_equal(values, m['values'])
    pos, nrm = xf.refine(I.grid('sphere16'), values, n, m['vert_edge'], sdf_p=(0.25, -0.5, 0.125))
    assert np.array_equal(pos, m['positions']) and np.array_equal(nrm, m['normals'])


def test_mesh_files_round_trip(host, tmp_path):
    """(f) save_ply / save_obj are read back by load_ply / load_obj."""
    import mesh_to_sdf as M
    m = host.mesh('sphere16', (16, 16, 16))
    v, f, nrm = m['positions'], m['faces'], m['normals']
    for normals in (None, nrm):
        fn = M.save_ply(str(tmp_path / 'a.ply'), v, f, normals)
        v2, f2 = M.load_ply(fn)
        assert np.array_equal(v2, v) and np.array_equal(f2, f)
        fn = M.save_obj(str(tmp_path / 'a.obj'), v, f, normals)
        v2, f2 = M.load_obj(fn)
        assert np.array_equal(v2, v) and np.array_equal(f2, f)
        assert np.array_equal(M.load_mesh(fn), v[f])
    fn = M.save_ply(str(tmp_path / 'empty.ply'), np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    v2, f2 = M.load_ply(fn)
    assert v2.shape == (0, 3) and f2.shape == (0, 3)
    with pytest.raises(ValueError, match='out of range'):
        M.save_ply(str(tmp_path / 'bad.ply'), v, f + len(v))


def test_argument_validation_before_device_work(built):
    """(g) the four entry points refuse bad arguments before any device work, and say who refused."""
    import dsdf
    lib = dsdf.load()
    one = C.c_void_p(16)                 # never dereferenced: validation fails first
    iso = C.c_float(0.0)
    sample = lambda *a: lib.dsdf_iso_sample(*a, None)
    mark = lambda *a: lib.dsdf_iso_mark(*a, None)
    emit = lambda *a: lib.dsdf_iso_emit(*a, None)
    refine = lambda *a: lib.dsdf_iso_refine(*a, None)
    cases = [
        (sample, (None, 8, 8, 8, 4, 4, 4, one), b'dsdf_iso_sample: null pointer'),
        (sample, (one, 8, 8, 8, 4, 4, 4, None), b'dsdf_iso_sample: null pointer'),
        (sample, (one, 8, 8, 8, 0, 4, 4, one), b'dsdf_iso_sample: the lattice needs'),
        (sample, (one, 8, 0, 8, 4, 4, 4, one), b'dsdf_iso_sample: bad grid size'),
        (sample, (one, 8, 8, 8, 512, 512, 512, one), b'dsdf_iso_sample: more than 2^27 lattice nodes'),
        (mark, (None, 4, 4, 4, iso, one, one, one), b'dsdf_iso_mark: null pointer'),
        (mark, (one, 4, 4, 4, iso, one, None, one), b'dsdf_iso_mark: null pointer'),
        (mark, (one, 4, -1, 4, iso, one, one, one), b'dsdf_iso_mark: the lattice needs'),
        (mark, (one, 1 << 27, 1, 1, iso, one, one, one), b'dsdf_iso_mark: more than 2^27 lattice nodes'),
        (emit, (one, 4, 4, 4, iso, None, one, one, one, one), b'dsdf_iso_emit: null pointer'),
        (emit, (one, 4, 4, 0, iso, one, one, one, one, one), b'dsdf_iso_emit: the lattice needs'),
        (emit, (one, 2048, 2048, 2048, iso, one, one, one, one, one), b'dsdf_iso_emit: more than 2^27 lattice nodes'),
        (refine, (one, 8, 8, 8, one, 4, 4, 4, iso, one, 5, 0, one, one), b'dsdf_iso_refine: steps must be 1 ... 32'),
        (refine, (one, 8, 8, 8, one, 4, 4, 4, iso, one, 5, 33, one, one), b'dsdf_iso_refine: steps must be 1 ... 32'),
        (refine, (one, 8, 8, 8, one, 4, 4, 4, iso, one, -1, 24, one, one), b'dsdf_iso_refine: negative vertex count'),
        (refine, (None, 8, 8, 8, one, 4, 4, 4, iso, one, 5, 24, one, one), b'dsdf_iso_refine: null pointer'),
        (refine, (one, 8, 8, 8, one, 4, 4, 4, iso, one, 5, 24, None, one), b'dsdf_iso_refine: null pointer'),
        (refine, (one, 8, 8, 8, one, 0, 4, 4, iso, one, 5, 24, one, one), b'dsdf_iso_refine: the lattice needs'),
        (refine, (one, 8, 8, 8, one, 512, 512, 512, iso, one, 5, 24, one, one), b'dsdf_iso_refine: more than 2^27 lattice nodes'),
        (refine, (one, 8, 8, 8, one, 4, 4, 4, iso, one, 7 * 125 + 1, 24, one, one), b'dsdf_iso_refine: more vertices than the lattice has edges'),
    ]
    for fn, args, text in cases:
        rc = fn(*args)
        assert rc == -1 and text in lib.dsdf_last_error(), (args, rc, lib.dsdf_last_error())
    # 512^3 cells is past the limit, 511^3 (2^27 nodes exactly) is not: the next check answers
    assert sample(None, 8, 8, 8, 511, 511, 511, one) == -1 and b'null pointer' in lib.dsdf_last_error()
    # no vertices: nothing to do, whatever the pointers
    assert refine(None, 8, 8, 8, None, 4, 4, 4, iso, None, 0, 24, None, None) == 0
    assert emit(one, 4, 4, 4, iso, one, one, one, None, None) == 0
    assert hasattr(dsdf, 'extract_mesh')


def _case_file(path, n, values, ref, iso=0.0, data=None):
    d = np.zeros((0, 0, 0), np.float32) if data is None else np.ascontiguousarray(data, np.float32)
    rz, ry, rx = d.shape
    with open(path, 'wb') as fh:
        fh.write(np.asarray(list(n) + [rx, ry, rz, len(ref['vert_edge']), len(ref['faces'])], np.int32).tobytes() + np.float32(iso).tobytes())
        fh.write(np.asarray(values, np.float32).tobytes() + ref['cross'].tobytes() + ref['n_vert'].tobytes() + ref['n_tri'].tobytes())
        fh.write(ref['vert_edge'].tobytes() + np.ascontiguousarray(ref['faces'], np.int32).tobytes() + d.tobytes())
    return str(path)


def test_standalone_program_under_sanitizers(host, tmp_path):
    """(h) the stand-alone program (its own main, nothing loaded into Python) built with AddressSanitizer + UBSan runs (a) clean: every
    value lattice, and every grid with its sampling and its vertices."""
    exe = sanitized_program('dsdf_iso_host.cpp')
    files = []
    for name, (n, values) in I.VALUE_LATTICES.items():
        files.append(_case_file(tmp_path / f'{name}.bin', n, values, I.topology(values, n)))
    for name, n in I.GRID_CASES.items():
        m = host.mesh(name, n)
        files.append(_case_file(tmp_path / f'{name}.bin', n, m['values'], I.topology(m['values'], n), data=I.grid(name)))
    for fn in files:
        run_case(exe, fn)
