"""CPU check of the mesh's connected components (csrc/dsdf_components.h: union-find over the index buffer, per-face area and volume
terms) through its stand-alone host build (tests/harness/dsdf_components_host.cpp) against the numpy reference in another formulation
(tests/mesh_components_oracle.py).

EXACT: label, and the numbering derived from it, are `==` the reference's on every case; where scipy imports, the partition is also the
one of scipy.sparse.csgraph.connected_components.
SUMS.  The fp64 sum of a component's F_c fp32 terms, in any order, lies within F_c 2^-53 sum |term| of the exact sum of the same terms
(every partial sum is bounded by sum |term| and each of the F_c additions rounds once): no measured gate.
GATE.  Against the all-fp64 measures the error is the fp32 rounding of the terms: mesh_components_oracle.MEASURED_MAX_ERR is the maximum
of |sum of fp32 terms - fp64 measure| / scale of the host build over the case table (scale: the area; for a volume the sum of
|p0| |p1| |p2| / 6 over the faces, since the term itself cancels for a triangle seen edge-on from the origin), the gate 4 x that, shared
with the GPU tests.  `PYTHONPATH=oracle:tests python tests/test_mesh_components_host.py` prints the measurements."""
import ctypes as C

import numpy as np
import pytest

import mesh_components_oracle as O
from host_build import ptr as _p, run_case, sanitized_program, shared_lib


def load_host():
    return shared_lib('dsdf_components_host.cpp')


@pytest.fixture(scope='module')
def host():
    return load_host()


def host_labels(host, f, V):
    """(label (V,) int32, status) of the host build."""
    f = np.ascontiguousarray(f, np.int32)
    label = np.full(V, -7, np.int32)
    status = np.zeros(1, np.int32)
    assert host.components_host(_p(f), C.c_long(len(f)), int(V), _p(label), _p(status)) == 0
    return label, int(status[0])


def host_measures(host, v, f):
    """The per-face (area, vol) of the host build, float32."""
    v, f = np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int32)
    area, vol = np.full(len(f), np.nan, np.float32), np.full(len(f), np.nan, np.float32)
    assert host.face_measures_host(_p(v), _p(f), C.c_long(len(f)), _p(area), _p(vol)) == 0
    return area, vol


def measure_errors(area32, vol32, ref):
    """(the two relative errors against the all-fp64 measures, whether the fp64 sums of the fp32 terms meet their bound) per component."""
    fc, n = ref['face_component'], ref['n']
    out = []
    for terms, exact, mag in ((area32, ref['area'], ref['abs_area']), (vol32, ref['volume'], ref['abs_volume'])):
        s, a, cnt = O.exact_sums(terms, fc, n)
        got = np.zeros(n)
        np.add.at(got, fc, terms.astype(np.float64))                       # fp64 sums in index order, as one order of many
        assert (np.abs(got - s) <= cnt * 2.0 ** -53 * a).all()
        out.append(float((np.abs(s - exact) / np.where(mag > 0, mag, 1.0)).max()) if n else 0.0)
    return out


@pytest.mark.parametrize('name', O.CASES)
def test_labels_and_numbering_equal_the_reference(host, name):
    v, f = O.mesh(name)
    ref = O.reference(name)
    label, status = host_labels(host, f, len(v))
    assert status == 0 and np.array_equal(label, ref['label'])
    n, fc, vc = O.numbering(label, f)
    assert (n, ref['n']) == (O.KNOWN[name][0],) * 2
    assert int((ref['boundary_edges'] == 0).sum()) == O.KNOWN[name][1]
    assert ((fc >= 0) & (fc < max(n, 1))).all() and ((vc >= -1) & (vc < max(n, 1))).all()
    if len(f):
        assert (vc[f] == fc[:, None]).all() and (label[f] == label[f[:, :1]]).all()
    named = np.zeros(len(v), bool)
    named[f.reshape(-1)] = True
    assert ((vc == -1) == ~named).all() and (label[~named] == np.nonzero(~named)[0]).all()
    assert (label <= np.arange(len(v))).all() and (label[label] == label).all()


@pytest.mark.parametrize('name', O.CASES)
def test_partition_equals_scipy(host, name):
    sp = pytest.importorskip('scipy.sparse')
    cg = pytest.importorskip('scipy.sparse.csgraph')
    v, f = O.mesh(name)
    V = len(v)
    if V == 0:
        return
    label, _ = host_labels(host, f, V)
    i, j = np.concatenate([f[:, 0], f[:, 1]]), np.concatenate([f[:, 1], f[:, 2]])
    n, theirs = cg.connected_components(sp.coo_matrix((np.ones(len(i)), (i, j)), shape=(V, V)), directed=False)
    assert n == len(np.unique(label))
    first = np.full(n, V)
    np.minimum.at(first, theirs, np.arange(V))
    assert np.array_equal(first[theirs], label)


def test_the_three_ribbons_are_one_surface(host):
    """Ascending, descending and permuted vertex numbers: one component each, and the labels are the smallest index whatever the depth
    of the chains the order of the unions builds."""
    for name in ('ribbon_asc', 'ribbon_desc', 'ribbon_perm'):
        v, f = O.mesh(name)
        label, status = host_labels(host, f, len(v))
        assert status == 0 and (label == 0).all()
    va, fa = O.mesh('ribbon_asc')
    vp, fp = O.mesh('ribbon_perm')
    assert np.array_equal(va[fa], vp[fp])


def test_unreferenced_vertices_do_not_shift_the_numbering(host):
    v, f = O.mesh('unreferenced')
    label, _ = host_labels(host, f, len(v))
    n, fc, vc = O.numbering(label, f)
    assert n == 2 and fc.tolist() == [0, 1]
    assert vc.tolist() == [-1, -1, 0, 0, 0, -1, -1, 1, 1, 1, -1] and label.tolist() == [0, 1, 2, 2, 2, 5, 6, 7, 7, 7, 10]


@pytest.mark.parametrize('name', [n for n in O.CASES if n != 'empty_0'])
def test_measures_against_fp64(host, name):
    v, f = O.mesh(name)
    ref = O.reference(name)
    area, vol = host_measures(host, v, f)
    assert (area >= 0).all() and np.isfinite(vol).all()
    ea, ev = measure_errors(area, vol, ref)
    print(f'{name}: C = {ref["n"]}; area error {ea:.3e}, volume error {ev:.3e} (relative to the sum of magnitudes)')
    assert ea <= O.GATE and ev <= O.GATE


def test_two_spheres_torus_and_sheet():
    ref = O.reference('two_spheres')
    assert ref['n'] == 2 and (ref['boundary_edges'] == 0).all()
    for c, (_, r) in enumerate(O.S.TWO):
        exact = 4.0 * np.pi * r ** 3 / 3.0
        print(f'sphere {c}: volume {ref["volume"][c]:.6f}, 4 pi r^3 / 3 = {exact:.6f}, ratio {ref["volume"][c] / exact:.5f}')
        assert abs(ref['volume'][c] / exact - 1.0) < 0.01
        assert abs(ref['area'][c] / (4.0 * np.pi * r ** 2) - 1.0) < 0.01
    torus, sheet = O.reference('torus'), O.reference('sheet')
    assert torus['n'] == 1 and torus['boundary_edges'].tolist() == [0] and torus['volume'][0] > 0
    assert abs(torus['volume'][0] / (2 * np.pi ** 2 * 0.3 * 0.1 ** 2) - 1.0) < 0.05
    assert sheet['n'] == 1 and sheet['boundary_edges'].tolist() == [4 * 12]


def test_give_up_on_a_label_array_with_a_cycle(host):
    """No input of dsdf_mesh_components makes a cycle; the cap that ends a walk through one is run here, on the host, only."""
    cyc = np.asarray([1, 2, 0, 3], np.int32)
    status = np.zeros(1, np.int32)
    assert host.root_host(_p(cyc), 0, 4, _p(status)) == -1 and status[0] == 1
    status[0] = 0
    assert host.root_host(_p(cyc), 3, 4, _p(status)) == 3 and status[0] == 0
    host.union_host(_p(cyc), 3, 1, 4, _p(status))
    assert status[0] == 1 and cyc.tolist() == [1, 2, 0, 3]
    chain = np.asarray([0, 0, 1, 2, 3], np.int32)                        # the deepest forest of 5: V reads, below the cap
    status[0] = 0
    assert host.root_host(_p(chain), 4, 5, _p(status)) == 0 and status[0] == 0


def test_refusals(host):
    f = np.zeros((1, 3), np.int32)
    label, status = np.zeros(4, np.int32), np.zeros(1, np.int32)
    assert host.components_host(_p(f), C.c_long(-1), 4, _p(label), _p(status)) == -1
    assert host.components_host(None, C.c_long(1), 4, _p(label), _p(status)) == -1
    assert host.components_host(_p(f), C.c_long(1), 4, None, _p(status)) == -1
    assert host.components_host(_p(f), C.c_long(1), 4, _p(label), None) == -1
    assert host.components_host(_p(f), C.c_long(1 << 30), 4, _p(label), _p(status)) == -1
    assert host.components_host(None, C.c_long(0), 0, None, None) == 0
    assert host.face_measures_host(None, None, C.c_long(0), None, None) == 0
    assert host.face_measures_host(None, _p(f), C.c_long(1), _p(label), _p(label)) == -1


def test_standalone_program_under_sanitizers(tmp_path):
    """The stand-alone program (its own main, nothing loaded into Python) built with AddressSanitizer + UBSan on the ribbons, the fans
    and the degenerate cases; it also walks the cycle."""
    exe = sanitized_program('dsdf_components_host.cpp')
    for name in O.DEGENERATE + ('ribbon_asc', 'ribbon_desc', 'ribbon_perm', 'fan_hub0', 'fan_hublast'):
        v, f = O.mesh(name)
        fn = tmp_path / f'{name}.bin'
        with open(fn, 'wb') as fh:
            fh.write(np.asarray([len(v), len(f)], np.int32).tobytes() + np.ascontiguousarray(v, np.float32).tobytes())
            fh.write(np.ascontiguousarray(f, np.int32).tobytes())
        run_case(exe, fn)


def test_python_layer_checks_that_need_no_device():
    import torch
    import dsdf
    import mesh_components
    f = torch.from_numpy(O.mesh('shared_edge')[1])
    with pytest.raises(dsdf.DsdfError, match='no CPU path'):
        dsdf.mesh_components(f)
    with pytest.raises(dsdf.DsdfError, match='connect'):
        dsdf.mesh_components(f, connect='edge')
    with pytest.raises(dsdf.DsdfError, match=r'\(F,3\)'):
        dsdf.mesh_components(f.reshape(-1))
    with pytest.raises(dsdf.DsdfError, match='keep'):
        dsdf.filter_components(torch.zeros(4, 3), f, keep=0)
    a = mesh_components.parse_args(['in.ply', '-o', 'out.ply', '--keep-largest', '2', '--min-area', '0.5', '--connect', 'position'])
    assert (a.input, a.output, a.keep_largest, a.min_area, a.min_faces, a.connect, a.json) == ('in.ply', 'out.ply', 2, 0.5, None, 'position', None)
    assert mesh_components.parse_args(['in.vol']).output is None
    for bad in ([], ['in.ply', '--keep-largest', '0'], ['in.ply', '--connect', 'edge'], ['in.ply', '-o', 'out.stl'], ['in.ply', '--min-area', '-1']):
        with pytest.raises(SystemExit) as e:
            mesh_components.parse_args(bad)
        assert e.value.code != 0
    import extract_mesh
    a = extract_mesh.parse_args(['g.vol', '--keep-largest'])
    assert a.keep_largest == 1 and a.min_component_area is None
    assert extract_mesh.parse_args(['g.vol', '--keep-largest', '3', '--min-component-area', '0.1']).keep_largest == 3
    assert extract_mesh.parse_args(['g.vol']).keep_largest is None


if __name__ == '__main__':
    h = load_host()
    worst = 0.0
    for nm in O.CASES:
        v_, f_ = O.mesh(nm)
        ea_, ev_ = measure_errors(*host_measures(h, v_, f_), O.reference(nm))
        print(f'{nm:16s} V = {len(v_):6d} F = {len(f_):6d} C = {O.reference(nm)["n"]:6d}: area {ea_:.3e}, volume {ev_:.3e}')
        worst = max(worst, ea_, ev_)
    print(f'MEASURED_MAX_ERR = {worst:.3e}; gate = 4 x = {4 * worst:.3e}')
