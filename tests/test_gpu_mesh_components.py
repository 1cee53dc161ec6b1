"""GPU checks of the mesh's connected components (include/dsdf.h: dsdf_mesh_components, dsdf_mesh_face_measures; dsdf.mesh_components,
dsdf.filter_components) against the HOST build of the same statements (tests/harness/dsdf_components_host.cpp) and the numpy reference
in another formulation (tests/mesh_components_oracle.py).

EXACT.  label is an exact function of the index buffer -- the smallest vertex index of each component -- whatever the order in which the
lanes win their compare-and-swaps: device label, face_component and vertex_component are `==` the host build's and the reference's, and
the per-face area / vol are the host build's BITS (uncontracted + - x / sqrtf).  A difference is a finding, not noise.
SUMS.  A component's float64 sum of its F_c float32 terms lies within F_c 2^-53 sum |term| of the exact sum of those terms, in any order.
GATE.  mesh_components_oracle.GATE = 4 x the maximum error of the host build against the all-fp64 measures (tests/
test_mesh_components_host.py); the device, summing the host's bits in fp64, has the host's error.
Measured on the MI355X: label, numbering and the per-face bits `==` the host build and the reference on all 24 cases; the float64 sums
against the all-fp64 measures: maximum 3.385e-06 (the area of a sliver in parts_20000, the host build's figure to every digit printed;
gate 1.354e-05), 5.608e-07 on disjoint_256, below 2e-07 on every other case."""
import ctypes as C

import numpy as np
import pytest
import torch

import mesh_components_oracle as O
from test_mesh_components_host import host_labels, host_measures, load_host

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dsdf(built):
    import dsdf as m
    m.load()
    assert torch.cuda.is_available()
    return m


@pytest.fixture(scope='module')
def host():
    return load_host()


def _cuda(a, dt=None):
    return torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()


def device_labels(dsdf, f, V):
    """(label, status) straight from dsdf_mesh_components."""
    lib = dsdf.load()
    faces = _cuda(f, np.int32)
    label = torch.full((V,), -7, dtype=torch.int32, device='cuda')
    status = torch.zeros(1, dtype=torch.int32, device='cuda')
    rc = lib.dsdf_mesh_components(C.c_void_p(faces.data_ptr()), len(f), V, C.c_void_p(label.data_ptr()), C.c_void_p(status.data_ptr()), None)
    assert rc == 0, lib.dsdf_last_error()
    torch.cuda.synchronize()
    return label.cpu().numpy(), int(status.item())


def device_measures(dsdf, v, f):
    lib = dsdf.load()
    vert, faces = _cuda(v, np.float32), _cuda(f, np.int32)
    area, vol = (torch.full((len(f),), float('nan'), device='cuda') for _ in range(2))
    rc = lib.dsdf_mesh_face_measures(C.c_void_p(vert.data_ptr()), C.c_void_p(faces.data_ptr()), len(f), C.c_void_p(area.data_ptr()),
                                     C.c_void_p(vol.data_ptr()), None)
    assert rc == 0, lib.dsdf_last_error()
    return area.cpu().numpy(), vol.cpu().numpy()


INT_FIELDS = ('label', 'face_component', 'vertex_component', 'faces_per_component', 'boundary_edges')


def as_numpy(comp):
    return {k: getattr(comp, k).cpu().numpy() for k in comp.__slots__ if isinstance(getattr(comp, k), torch.Tensor)}


# ---- every case of the table ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', O.CASES)
def test_device_equals_host_build_and_reference(dsdf, host, name):
    v, f = O.mesh(name)
    V = len(v)
    ref = O.reference(name)
    label, status = device_labels(dsdf, f, V)
    hlabel, hstatus = host_labels(host, f, V)
    assert status == 0 == hstatus
    assert np.array_equal(label, hlabel) and np.array_equal(label, ref['label'])
    area, vol = device_measures(dsdf, v, f)
    harea, hvol = host_measures(host, v, f)
    assert np.array_equal(area.view(np.int32), harea.view(np.int32)) and np.array_equal(vol.view(np.int32), hvol.view(np.int32))

    comp = dsdf.mesh_components(_cuda(f, np.int32), vertices=_cuda(v, np.float32))
    got = as_numpy(comp)
    assert comp.n == ref['n'] == O.KNOWN[name][0]
    for k in INT_FIELDS:
        assert got[k].shape == ref[k].shape and np.array_equal(got[k], ref[k]), (name, k)
    assert comp.label.dtype == comp.face_component.dtype == comp.vertex_component.dtype == torch.int32
    assert comp.faces_per_component.dtype == comp.boundary_edges.dtype == torch.int64
    assert comp.area.dtype == comp.volume.dtype == torch.float64 and comp.bbox.dtype == torch.float32
    assert got['bbox'].shape == (comp.n, 2, 3) and np.array_equal(got['bbox'], ref['bbox'])
    worst = 0.0
    for terms, key, scale in ((area, 'area', 'abs_area'), (vol, 'volume', 'abs_volume')):
        exact, mag, count = O.exact_sums(terms, ref['face_component'], comp.n)
        assert got[key].shape == (comp.n,) and (np.abs(got[key] - exact) <= count * 2.0 ** -53 * mag).all(), (name, key)
        if comp.n:
            worst = max(worst, float((np.abs(got[key] - ref[key]) / np.where(ref[scale] > 0, ref[scale], 1.0)).max()))
    print(f'{name}: C = {comp.n}; device sums against the all-fp64 measures: {worst:.3e} (gate {O.GATE:.3e})')
    assert worst <= O.GATE

    # a second call returns the same tensors; int64 faces, and the count alone instead of the vertices, change nothing
    again = as_numpy(dsdf.mesh_components(_cuda(f, np.int64), n_vertices=V))
    for k in ('label', 'face_component', 'vertex_component', 'faces_per_component'):
        assert np.array_equal(again[k], got[k]), (name, k)
    assert 'area' not in again and 'boundary_edges' not in again
    twice = as_numpy(dsdf.mesh_components(_cuda(f, np.int32), vertices=_cuda(v, np.float32)))
    for k in INT_FIELDS + ('bbox',):
        assert np.array_equal(twice[k], got[k]), (name, k)


def test_ribbons_in_three_numberings_are_one_partition(dsdf):
    """Ascending, descending and permuted vertex numbers build chains of very different depth; the partition of the faces is the same."""
    for name in ('ribbon_asc', 'ribbon_desc', 'ribbon_perm'):
        v, f = O.mesh(name)
        comp = dsdf.mesh_components(_cuda(f, np.int32))
        assert comp.n == 1 and int(comp.label.max()) == 0 and int(comp.face_component.max()) == 0 and int(comp.vertex_component.min()) == 0


def test_default_vertex_count_is_the_largest_index_plus_one(dsdf):
    v, f = O.mesh('unreferenced')
    comp = dsdf.mesh_components(_cuda(f, np.int32))
    assert comp.label.tolist() == [0, 1, 2, 2, 2, 5, 6, 7, 7, 7] and comp.vertex_component.tolist() == [-1, -1, 0, 0, 0, -1, -1, 1, 1, 1]
    comp = dsdf.mesh_components(_cuda(f, np.int32), n_vertices=11)
    assert comp.vertex_component.tolist() == [-1, -1, 0, 0, 0, -1, -1, 1, 1, 1, -1] and comp.area is None and comp.bbox is None
    empty = dsdf.mesh_components(torch.zeros(0, 3, dtype=torch.int32, device='cuda'))
    assert empty.n == 0 and empty.label.shape == (0,) and empty.face_component.shape == (0,) and empty.faces_per_component.shape == (0,)


# ---- a soup with repeated vertices ---------------------------------------------------------------------------------------------------
def test_soup_by_index_and_by_position(dsdf):
    v, f = O.mesh('sphere_soup')
    vert, faces = _cuda(v, np.float32), _cuda(f, np.int32)
    by_index = dsdf.mesh_components(faces, vertices=vert)
    assert by_index.n == len(f) and by_index.face_component.tolist() == list(range(len(f)))
    welded = dsdf.mesh_components(faces, vertices=vert, connect='position')
    assert welded.n == 1 and welded.boundary_edges.tolist() == [0] and welded.faces_per_component.tolist() == [len(f)]
    assert welded.label.shape == (len(v),) and int(welded.label.max()) == 0                    # the caller's numbering
    assert welded.face_component.shape == (len(f),) and int(welded.face_component.max()) == 0 and int(welded.vertex_component.min()) == 0
    sv, sf = O.S.mesh('sphere')
    ref_area, ref_vol = (t.sum() for t in O.face_measures64(sv, sf))
    assert abs(float(welded.area[0]) - ref_area) <= O.GATE * ref_area and abs(float(welded.volume[0]) - ref_vol) <= O.GATE * O.volume_scale(sv, sf).sum()
    # on a mesh without repeated positions both ways agree, and the components keep the order of the caller's smallest index
    v2, f2 = O.mesh('two_spheres')
    a = as_numpy(dsdf.mesh_components(_cuda(f2, np.int32), vertices=_cuda(v2, np.float32)))
    b = as_numpy(dsdf.mesh_components(_cuda(f2, np.int32), vertices=_cuda(v2, np.float32), connect='position'))
    for k in INT_FIELDS + ('bbox',):
        assert np.array_equal(a[k], b[k]), k


# ---- filter_components ------------------------------------------------------------------------------------------------------------------
def test_keep_the_largest_of_two_spheres(dsdf):
    v, f = O.mesh('two_spheres')
    ref = O.reference('two_spheres')
    big = int(np.argmax(ref['area']))
    assert big == 0                                                                  # radius 0.3 before radius 0.25
    vert, faces = _cuda(v, np.float32), _cuda(f, np.int32)
    nrm = torch.nn.functional.normalize(vert - vert.mean(0), dim=1)
    col = torch.rand(len(v), 3, device='cuda', generator=torch.Generator(device='cuda').manual_seed(2))
    vo, fo, no, co = dsdf.filter_components(vert, faces, keep=1, normals=nrm, colors=col)
    stays = ref['face_component'] == big
    assert vo.dtype == torch.float32 and fo.dtype == torch.int32 and fo.shape == (int(stays.sum()), 3)
    named = np.unique(f[stays])
    assert np.array_equal(vo.cpu().numpy(), v[named]) and np.array_equal(no.cpu().numpy(), nrm.cpu().numpy()[named])
    assert np.array_equal(co.cpu().numpy(), col.cpu().numpy()[named])
    assert np.array_equal(vo.cpu().numpy()[fo.cpu().numpy()], v[f[stays]])           # the faces in input order with their winding
    again = dsdf.mesh_components(fo, vertices=vo)
    assert again.n == 1 and again.boundary_edges.tolist() == [0]
    area_in, _ = device_measures(dsdf, v, f)
    area_out, _ = device_measures(dsdf, vo.cpu().numpy(), fo.cpu().numpy())
    assert np.array_equal(area_out.view(np.int32), area_in[stays].view(np.int32))
    # keep = 2 keeps all; the thresholds combine with keep by AND; the small sphere alone through min_area / min_faces is not reachable,
    # the large one is
    assert dsdf.filter_components(vert, faces, keep=2)[1].shape == faces.shape and dsdf.filter_components(vert, faces, keep=5)[1].shape == faces.shape
    between = float(ref['area'].min() + ref['area'].max()) / 2
    v1, f1, counts = dsdf.filter_components(vert, faces, min_area=between, return_counts=True)
    assert counts == (2, 1) and torch.equal(f1, fo) and torch.equal(v1, vo)
    assert dsdf.filter_components(vert, faces, keep=2, min_area=between)[1].shape == fo.shape
    assert dsdf.filter_components(vert, faces, min_faces=int(stays.sum()))[1].shape == faces.shape       # both spheres have that many


def test_everything_filtered_away(dsdf):
    v, f = O.mesh('two_spheres')
    vert, faces = _cuda(v, np.float32), _cuda(f, np.int32)
    out = dsdf.filter_components(vert, faces, min_area=1e9, normals=vert, colors=vert)
    assert len(out) == 4 and all(tuple(t.shape) == (0, 3) and t.is_cuda for t in out)
    assert out[1].dtype == torch.int32 and out[0].dtype == torch.float32
    out = dsdf.filter_components(vert, faces[:0], keep=1)
    assert len(out) == 2 and all(tuple(t.shape) == (0, 3) for t in out)
    out = dsdf.filter_components(vert, faces, min_faces=10 ** 7)
    assert all(tuple(t.shape) == (0, 3) for t in out)


def test_ties_go_to_the_smaller_component_number(dsdf):
    """Two copies of one triangle, bit for bit: equal areas; keep = 1 keeps the first."""
    v = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0]])
    vert, faces = _cuda(np.concatenate([v, v])), _cuda(np.int32([[0, 1, 2], [3, 4, 5]]))
    vo, fo = dsdf.filter_components(vert, faces, keep=1)
    assert fo.tolist() == [[0, 1, 2]] and vo.shape == (3, 3)
    vo, fo = dsdf.filter_components(vert, _cuda(np.int32([[3, 4, 5], [0, 1, 2]])), keep=1)
    assert fo.tolist() == [[0, 1, 2]] and vo.shape == (3, 3)                         # component 0 is the one with vertex 0: the second face


# ---- arguments ---------------------------------------------------------------------------------------------------------------------------
def test_argument_validation(dsdf):
    lib = dsdf.load()
    one = C.c_void_p(16)            # never dereferenced: validation fails first
    for args in ((None, 8, 4, one, one), (one, 8, 4, None, one), (one, 8, 4, one, None), (one, -1, 4, one, one), (one, 8, -1, one, one),
                 (one, 1 << 30, 4, one, one)):
        assert lib.dsdf_mesh_components(*args, None) == -1 and lib.dsdf_last_error().startswith(b'dsdf_mesh_components'), args
    assert lib.dsdf_mesh_components(None, 0, 0, None, None, None) == 0                # no vertices: no launch, no pointers
    for args in ((None, one, 8, one, one), (one, None, 8, one, one), (one, one, 8, None, one), (one, one, 8, one, None), (one, one, -1, one, one),
                 (one, one, 1 << 30, one, one)):
        assert lib.dsdf_mesh_face_measures(*args, None) == -1 and lib.dsdf_last_error().startswith(b'dsdf_mesh_face_measures'), args
    assert lib.dsdf_mesh_face_measures(None, None, 0, None, None, None) == 0
    v, f = (_cuda(a, dt) for a, dt in zip(O.mesh('torus'), (np.float32, np.int32)))
    mc, fc = dsdf.mesh_components, dsdf.filter_components
    for call in (lambda: mc(f.cpu()), lambda: mc(f, vertices=v.cpu()), lambda: fc(v.cpu(), f), lambda: fc(v, f.cpu()),
                 lambda: fc(v, f, normals=v.cpu()), lambda: fc(v, f, colors=v.cpu())):
        with pytest.raises(dsdf.DsdfError, match='no CPU path'):
            call()
    for call in (lambda: mc(f.reshape(-1)), lambda: mc(f[:, :2]), lambda: fc(v, f.reshape(-1))):
        with pytest.raises(dsdf.DsdfError, match=r'\(F,3\)'):
            call()
    for call in (lambda: mc(f, vertices=v.reshape(-1)), lambda: fc(v[:, :2], f), lambda: fc(None, f)):
        with pytest.raises(dsdf.DsdfError, match=r'\(V,3\)'):
            call()
    for call in (lambda: mc(f.float()), lambda: fc(v, f.short())):
        with pytest.raises(dsdf.DsdfError, match='int32'):
            call()
    for call in (lambda: mc(f, vertices=v.double()), lambda: fc(v.double(), f), lambda: fc(v, f, colors=v.double())):
        with pytest.raises(dsdf.DsdfError, match='float32'):
            call()
    for call in (lambda: mc(f, vertices=v[:100]), lambda: mc(f, n_vertices=100), lambda: mc(f - 1), lambda: fc(v[:100], f), lambda: fc(v, f - 1)):
        with pytest.raises(dsdf.DsdfError, match='out of range'):
            call()
    with pytest.raises(dsdf.DsdfError, match='n_vertices'):
        mc(f, n_vertices=len(v) + 1, vertices=v)
    with pytest.raises(dsdf.DsdfError, match='n_vertices'):
        mc(f[:0], n_vertices=-1)
    for call in (lambda: mc(f, connect='edge'), lambda: fc(v, f, connect='edge')):
        with pytest.raises(dsdf.DsdfError, match='connect'):
            call()
    with pytest.raises(dsdf.DsdfError, match='needs the vertices'):
        mc(f, connect='position')
    for bad in (0, -1, 1.5, True):
        with pytest.raises(dsdf.DsdfError, match='keep'):
            fc(v, f, keep=bad)
    for bad in (-1.0, float('nan')):
        with pytest.raises(dsdf.DsdfError, match='min_area'):
            fc(v, f, min_area=bad)
    for bad in (-1, 2.5):
        with pytest.raises(dsdf.DsdfError, match='min_faces'):
            fc(v, f, min_faces=bad)
    with pytest.raises(dsdf.DsdfError, match='normals'):
        fc(v, f, normals=v[:10])
    with pytest.raises(dsdf.DsdfError, match='colors'):
        fc(v, f, colors=v[:10])
