"""CPU check of the mesh simplification (csrc/dsdf_simplify.h: vertex clustering with quadric error metrics) through its stand-alone host
build (tests/harness/dsdf_simplify_host.cpp) against the fp64 reference in another formulation (tests/mesh_simplify_oracle.py).

EXACT: the cell key of every face corner, the output faces and the number of output vertices are `==` the reference's.
GATE.  The fp32 error of the positions was measured, not guessed: max |x_fp32 - x_fp64| / cell size (per axis) of the host build over the
case table is mesh_simplify_oracle.MEASURED_MAX_ERR; the gate is 4 x that, shared with the GPU tests, and also bounds the error of the
normals and of the colours (both are of order 1).
GUARANTEES.  1: every point of the output lies within one cell diagonal D of the input surface (every output face is an input face with
its corners moved inside their cells).  2: on a closed mesh the winding number of the output equals the input's as an integer at every
point farther than D from the input surface.  3: in a cell that holds a corner of the cube the representative lies within 0.01 D of it.
`PYTHONPATH=oracle:tests python tests/test_mesh_simplify_host.py` prints the measurements (profiles/mesh_simplify.md holds them)."""
import ctypes as C

import numpy as np
import pytest

import mesh_closest_oracle as CO
import mesh_simplify_oracle as O
import mesh_winding_oracle as WO
from host_build import ptr as _p, run_case, sanitized_program, shared_lib

GATE = O.GATE


def load_host():
    return shared_lib('dsdf_simplify_host.cpp')


@pytest.fixture(scope='module')
def host():
    return load_host()


def simplify(host, v, f, lo, hi, cells, reg=O.REG, colors=None, normals=True):
    """The host build's result as a dict like the oracle's (fp32 arrays), or the text of its refusal."""
    v = None if v is None else np.ascontiguousarray(v, np.float32)
    f = None if f is None else np.ascontiguousarray(f, np.int32)
    F = 0 if f is None else f.shape[0]
    lo = None if lo is None else np.ascontiguousarray(lo, np.float32)
    hi = None if hi is None else np.ascontiguousarray(hi, np.float32)
    col = None if colors is None else np.ascontiguousarray(colors, np.float32)
    keys, fo = np.full((F, 3), -1, np.int32), np.full((F, 3), -1, np.int32)
    pos, nrm, co = (np.full((3 * F, 3), np.nan, np.float32) for _ in range(3))
    counts = (C.c_long * 3)()
    why = C.c_char_p()
    rc = host.simplify_host(_p(v), _p(f), C.c_long(F), _p(col), _p(lo), _p(hi), int(cells[0]), int(cells[1]), int(cells[2]), C.c_float(reg),
                            _p(keys), _p(fo), _p(pos), _p(nrm) if normals else None, _p(co) if col is not None else None, counts, C.byref(why))
    if rc != 0:
        return why.value.decode()
    nv, nf, U = counts[0], counts[1], counts[2]
    return dict(keys=keys, vertices=pos[:nv], faces=fo[:nf], normals=nrm[:nv] if normals else None, colors=co[:nv] if col is not None else None,
                occupied=U)


_cache = {}


def case(host, name):
    """(vertices, faces, (lo, hi), cells, host result, fp64 reference) of one case, computed once."""
    if name not in _cache:
        mname, (lo, hi), cells = O.CASES[name]
        v, f = O.mesh(mname)
        _cache[name] = (v, f, (lo, hi), cells, simplify(host, v, f, lo, hi, cells, colors=O.colors_of(v)), O.reference(name))
    return _cache[name]


def position_error(got, ref, box, cells):
    """max over vertices and axes of |x_fp32 - x_fp64| / cell size."""
    if len(ref['vertices']) == 0:
        return 0.0
    return float((np.abs(got['vertices'].astype(np.float64) - ref['vertices']) / O.cell_size(box[0], box[1], cells)).max())


@pytest.mark.parametrize('name', list(O.CASES))
def test_matches_fp64_reference(host, name):
    v, f, box, cells, got, ref = case(host, name)
    assert np.array_equal(got['keys'], ref['keys'])
    assert got['vertices'].shape == ref['vertices'].shape and np.array_equal(got['faces'], ref['faces'])
    assert got['occupied'] == len(np.unique(ref['keys']))
    err = position_error(got, ref, box, cells)
    nerr = float(np.abs(got['normals'] - ref['normals']).max()) if len(ref['vertices']) else 0.0
    cerr = float(np.abs(got['colors'] - ref['colors']).max()) if len(ref['vertices']) else 0.0
    print(f'{name}: {len(f)} -> {len(ref["faces"])} faces, {len(ref["vertices"])} vertices, {int(ref["clamped"].sum())} clamped; '
          f'max |x_fp32 - x_fp64| / cell = {err:.3e}, normals {nerr:.3e}, colours {cerr:.3e}')
    assert err <= GATE and nerr <= GATE and cerr <= GATE
    if name == 'collapse_1':
        assert got['vertices'].shape == (0, 3) and got['faces'].shape == (0, 3) and got['occupied'] == 1
    else:
        assert 0 < len(ref['faces']) < len(f)
    if name == 'degenerate_3':                                   # the vertex in front that no face uses took no part
        assert ref['keys'].min() >= 0 and 0 not in f and len(v) == f.max() + 1


@pytest.mark.parametrize('name', [n for n in O.CASES if n != 'collapse_1'])
def test_structure_of_the_output(host, name):
    """Vertices in ascending cell key and inside their cell's closed box; faces = the survivors in input order, winding kept."""
    v, f, box, cells, got, ref = case(host, name)
    lo, hi, c = O.grid_of(box[0], box[1], cells)
    size = O.cell_size(lo, hi, c)
    key = ref['cell']
    assert (np.diff(key) > 0).all()
    ijk = np.stack([key % c[0], (key // c[0]) % c[1], key // (c[0] * c[1])], -1)
    blo = lo.astype(np.float64) + ijk * size
    x = got['vertices'].astype(np.float64)
    tol = GATE * size                                             # (the fp32 rounding of the cell's own faces)
    assert (x >= blo - tol).all() and (x <= blo + size + tol).all()
    # every output face is the input face ref['kept'][j] with corner k moved into the cell of that corner
    assert np.array_equal(key[got['faces']], ref['keys'][ref['kept']])
    t = got['faces']
    assert (t[:, 0] != t[:, 1]).all() and (t[:, 1] != t[:, 2]).all() and (t[:, 2] != t[:, 0]).all()


@pytest.mark.parametrize('name', [n for n in O.CASES if n != 'collapse_1'])
def test_guarantee_1_output_within_one_diagonal_of_the_input(host, name):
    v, f, box, cells, got, ref = case(host, name)
    D = O.diagonal(box[0], box[1], cells)
    pts = O.sample_surface(got['vertices'], got['faces'], 2000, len(name))
    d = CO.closest(pts, v[f])[0].max()
    back = CO.closest(O.sample_surface(v, f, 2000, 1 + len(name)), got['vertices'][got['faces']])[0].max()
    print(f'{name}: output -> input {d / D:.3f} D, input -> output {back / D:.3f} D (sampled)')
    assert d <= D + GATE * np.linalg.norm(O.cell_size(box[0], box[1], cells))


@pytest.mark.parametrize('name', O.CLOSED)
def test_guarantee_2_winding_number_is_kept(host, name):
    v, f, box, cells, got, ref = case(host, name)
    D = O.diagonal(box[0], box[1], cells)
    rng = np.random.default_rng(len(name))
    inner = rng.uniform(-0.12, 0.12, (150, 3)) + np.asarray(O.SPHERE_C if name.startswith('sphere') else (0.0, 0.0, 0.0))
    pts = np.concatenate([rng.uniform(-1.0, 1.0, (450, 3)), inner])
    far = CO.closest(pts, v[f])[0] > D
    pts = pts[far]
    assert len(pts) >= 200, len(pts)
    w_in, w_out = WO.winding(pts, v[f]), WO.winding(pts, got['vertices'][got['faces']])
    print(f'{name}: {len(pts)} points farther than D = {D:.3f}, {int((np.rint(w_in) != 0).sum())} of them inside; '
          f'max |w - rint(w)| = {np.abs(w_out - np.rint(w_out)).max():.2e}')
    assert np.array_equal(np.rint(w_in), np.rint(w_out))
    assert np.abs(w_in - np.rint(w_in)).max() < 1e-6 and np.abs(w_out - np.rint(w_out)).max() < 1e-6


@pytest.mark.parametrize('name', ['cube_5', 'cube_7'])
def test_guarantee_3_corners_of_the_cube_stay(host, name):
    v, f, box, cells, got, ref = case(host, name)
    D = O.diagonal(box[0], box[1], cells)
    corners = np.asarray([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], np.float64) * 0.4 + np.asarray([0.013, -0.007, 0.021])
    keys = O.cell_keys(O.vertex_cells(corners, box[0], box[1], cells), np.asarray(cells))
    worst = 0.0
    for corner, key in zip(corners, keys):
        r = np.searchsorted(ref['cell'], key)
        assert ref['cell'][r] == key and not ref['clamped'][r]
        worst = max(worst, np.linalg.norm(got['vertices'][r].astype(np.float64) - corner) / D)
    print(f'{name}: corner miss <= {worst:.2e} D')
    assert worst <= 0.01


def test_normals(host):
    """Sphere: outward.  Cube: a cell that only holds triangles of one side has exactly that side's normal."""
    v, f, box, cells, got, ref = case(host, 'sphere_6')
    out = got['vertices'].astype(np.float64) - np.asarray(O.SPHERE_C)
    cosine = (got['normals'] * out).sum(1) / np.linalg.norm(out, axis=1)
    assert cosine.min() > 0.9 and np.abs(np.linalg.norm(got['normals'], axis=1) - 1).max() <= GATE
    v, f, box, cells, got, ref = case(host, 'cube_7')
    t = v[f].astype(np.float64)
    fn = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    fn /= np.linalg.norm(fn, axis=1, keepdims=True)
    interior = 0
    for r, key in enumerate(ref['cell']):
        ns = np.unique(np.rint(fn[np.nonzero(ref['keys'] == key)[0]]), axis=0)
        if len(ns) == 1:
            interior += 1
            assert np.abs(got['normals'][r] - ns[0]).max() <= GATE
    assert interior >= 6


@pytest.mark.parametrize('name', ['sphere_6', 'sheet_5', 'degenerate_3'])
def test_colors_of_an_affine_field(host, name):
    v, f, box, cells, got, ref = case(host, name)
    assert np.abs(got['colors'] - O.color_field(ref['mean'])).max() <= GATE
    plain = simplify(host, v, f, box[0], box[1], cells, normals=False)
    assert plain['colors'] is None and plain['normals'] is None and np.array_equal(plain['vertices'], got['vertices'])


@pytest.mark.parametrize('name', ['sphere_11', 'torus_9x9x5', 'degenerate_3'])
def test_permuting_the_faces(host, name):
    v, f, box, cells, got, ref = case(host, name)
    perm = np.random.default_rng(7).permutation(len(f))
    other = simplify(host, v, f[perm], box[0], box[1], cells)
    assert other['vertices'].shape == got['vertices'].shape
    assert sorted(map(tuple, other['faces'].tolist())) == sorted(map(tuple, got['faces'].tolist()))
    size = O.cell_size(box[0], box[1], cells)
    assert (np.abs(other['vertices'].astype(np.float64) - got['vertices']) / size).max() <= GATE


def test_flat_mesh_stays_in_its_plane(host):
    v, f, box, cells, got, ref = case(host, 'flat_4')
    size = O.cell_size(box[0], box[1], cells)
    assert np.abs(got['vertices'][:, 2].astype(np.float64) - 0.0625).max() <= GATE * size[2]
    assert np.abs(got['normals'] - np.float32([0, 0, 1])).max() <= GATE


def test_no_faces_and_refusals(host):
    v, f = O.mesh('sphere')
    lo, hi = O.UNIT
    empty = simplify(host, v, f[:0], lo, hi, (4, 4, 4))
    assert empty['vertices'].shape == (0, 3) and empty['faces'].shape == (0, 3) and empty['occupied'] == 0
    assert simplify(host, None, None, lo, hi, (4, 4, 4))['occupied'] == 0               # F = 0: no pointers needed
    assert '2^31' in simplify(host, v, f, lo, hi, (2048, 1024, 1024))
    assert '2^31' in simplify(host, v, f, lo, hi, (1 << 16, 1 << 16, 1))
    assert simplify(host, v, f, lo, hi, (1290, 1290, 1290))['occupied'] > 0               # 2146689000 < 2^31
    assert '>= 1' in simplify(host, v, f, lo, hi, (4, 0, 4))
    for bad_hi in ((0.5, -0.5, 0.5), (0.5, 0.5, -0.6), (np.nan, 0.5, 0.5), (np.inf, 0.5, 0.5)):
        assert 'lo < hi' in simplify(host, v, f, lo, bad_hi, (4, 4, 4))
    assert 'null' in simplify(host, v, f, None, hi, (4, 4, 4)) and 'null' in simplify(host, v, f, lo, None, (4, 4, 4))
    assert simplify(host, None, f, lo, hi, (4, 4, 4)) == 'bad argument' and simplify(host, v, None, lo, hi, (4, 4, 4))['occupied'] == 0
    for reg in (0.0, -1.0, float('nan')):
        assert 'reg' in simplify(host, v, f, lo, hi, (4, 4, 4), reg=reg)


def test_standalone_program_under_sanitizers(tmp_path):
    """The stand-alone program (its own main, nothing loaded into Python) built with AddressSanitizer + UBSan over every mesh of the table,
    and over one with a NaN and an infinite vertex."""
    exe = sanitized_program('dsdf_simplify_host.cpp')
    runs = [(n,) + O.mesh(m) + (b, c) for n, (m, b, c) in O.CASES.items()]
    v, f = O.mesh('sphere')
    v = v.copy()
    v[5], v[77, 1] = np.nan, np.inf
    runs.append(('nonfinite', v, f, O.UNIT, (6, 6, 6)))
    for name, v, f, (lo, hi), cells in runs:
        fn = tmp_path / f'{name}.bin'
        with open(fn, 'wb') as fh:
            fh.write(np.asarray([len(v), len(f)] + list(cells), np.int32).tobytes() + np.asarray(lo + hi, np.float32).tobytes())
            fh.write(np.ascontiguousarray(v, np.float32).tobytes() + np.nan_to_num(O.colors_of(v)).tobytes() + np.ascontiguousarray(f, np.int32).tobytes())
        run_case(exe, fn, verdict=' 0 failures')


def test_python_layer_checks_that_need_no_device():
    """simplify_mesh refuses CPU tensors like every other call; the two command lines parse before any device work."""
    import torch
    import dsdf
    import simplify_mesh
    v, f = O.mesh('sphere')
    with pytest.raises(dsdf.DsdfError, match='no CPU path'):
        dsdf.simplify_mesh(torch.from_numpy(v), torch.from_numpy(f.astype(np.int32)), 4)
    a = simplify_mesh.parse_args(['in.ply', 'out.obj', '--cells', '24'])
    assert (a.input, a.output, a.cells, a.reg) == ('in.ply', 'out.obj', 24, 1e-3)
    for bad in (['in.ply'], ['in.ply', 'out.ply'], ['in.ply', 'out.ply', '--cells', '0'], ['in.ply', 'out.stl', '--cells', '4']):
        with pytest.raises(SystemExit) as e:
            simplify_mesh.parse_args(bad)
        assert e.value.code != 0
    assert dsdf.renderer.resolve_cells(4, (0.0, 0.0, 0.0), (1.0, 0.5, 0.26)) == (4, 2, 2)
    assert dsdf.renderer.resolve_cells(7, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)) == (7, 7, 7)
    assert dsdf.renderer.resolve_cells((3, 4, 5), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)) == (3, 4, 5)
    assert dsdf.renderer.resolve_cells(8, (0.0, 0.0, 0.0), (1.0, 1e-9, 0.0 + 1e-4)) == (8, 1, 1)
    with pytest.raises(dsdf.DsdfError, match='cells'):
        dsdf.renderer.resolve_cells(0, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))


if __name__ == '__main__':
    h = load_host()
    worst = 0.0
    for nm in O.CASES:
        v_, f_, box_, cells_, got_, ref_ = case(h, nm)
        e = position_error(got_, ref_, box_, cells_)
        print(f'{nm:14s} {len(f_):5d} -> {len(ref_["faces"]):4d} faces, {len(ref_["vertices"]):4d} vertices, {int(ref_["clamped"].sum())} clamped: '
              f'max |x_fp32 - x_fp64| / cell = {e:.3e}')
        worst = max(worst, e)
    print(f'MEASURED_MAX_ERR = {worst:.3e}; gate = 4 x = {4 * worst:.3e}')
