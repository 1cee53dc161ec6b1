"""CPU check of the mesh BVH (csrc/dsdf_bvh.h) through its stand-alone host build (tests/harness/dsdf_bvh_host.cpp): the stackless
traversal must return BITWISE the same t, back-face flag and primitive index as a loop over all triangles with the same triangle
function -- on buffers written by a numpy builder from the layout documented in include/dsdf.h, and on buffers written by the
library's own per-element build statements run serially."""
import ctypes as C

import numpy as np
import pytest

from host_build import ptr as _p, run_case, sanitized_program, shared_lib
from mesh_bvh_cases import MESHES, morton_order, n_leaves, numpy_bvh, ray_sets


@pytest.fixture(scope='module')
def host():
    return shared_lib('dsdf_bvh_host.cpp', long_returning=['bvh_host_size'])


def cast_both(host, buf, tri, o, d, t_min):
    n = o.shape[0]
    res = []
    for which in ('bvh', 'brute'):
        t = np.zeros(n, np.float32); back = np.zeros(n, np.int32); prim = np.zeros(n, np.int32)
        if which == 'bvh':
            host.bvh_host_raycast(_p(buf), _p(o), _p(d), C.c_long(n), C.c_float(t_min), _p(t), _p(back), _p(prim))
        else:
            host.bvh_host_brute(_p(tri), int(tri.shape[0]), _p(o), _p(d), C.c_long(n), C.c_float(t_min), _p(t), _p(back), _p(prim))
        res.append((t, back, prim))
    return res


@pytest.mark.parametrize('builder', ['numpy', 'library'])
@pytest.mark.parametrize('name', list(MESHES))
def test_traversal_is_bitwise_brute_force(host, name, builder):
    tri = MESHES[name]
    T = tri.shape[0]
    assert host.bvh_host_size(T, 0) == 64 * n_leaves(T) and host.bvh_host_size(T, 1) == 100 * n_leaves(T)
    order = morton_order(tri)
    if builder == 'numpy':
        buf = numpy_bvh(tri, order)
    else:
        buf = np.full(64 * n_leaves(T), np.nan, np.float32)                  # (the build must write every float it relies on)
        host.bvh_host_build(_p(tri), None, _p(order), T, _p(buf))
        ref = numpy_bvh(tri, order)
        assert np.array_equal(buf.view(np.int32), ref.view(np.int32)), 'the build statements write the documented layout'
    hits = 0
    for rs, (o, d, t_min) in ray_sets(tri, len(name)).items():
        (t, back, prim), (t_ref, back_ref, prim_ref) = cast_both(host, buf, tri, o, d, t_min)
        assert np.array_equal(t.view(np.int32), t_ref.view(np.int32)), (name, rs)
        assert np.array_equal(back, back_ref) and np.array_equal(prim, prim_ref), (name, rs)
        assert (t[np.isfinite(t)] > t_min).all() and (prim[~np.isfinite(t)] == -1).all()
        if rs == 'miss_root':
            assert not np.isfinite(t).any()
        hits += int(np.isfinite(t).sum())
    assert hits > 100 or T < 4                                               # the rays do meet the mesh


def test_given_order_and_anyhit(host):
    """order = NULL keeps the given order; the any-hit query agrees with the closest hit about `a hit below t_max`."""
    tri = MESHES['ico320']
    T = tri.shape[0]
    buf = np.zeros(64 * n_leaves(T), np.float32)
    host.bvh_host_build(_p(tri), None, None, T, _p(buf))
    assert np.array_equal(buf.view(np.int32), numpy_bvh(tri).view(np.int32))
    o, d, _ = ray_sets(tri, 3)['random']
    (t, _, _), (t_ref, _, _) = cast_both(host, buf, tri, o, d, 0.0)
    assert np.array_equal(t.view(np.int32), t_ref.view(np.int32))
    t_max = np.where(np.arange(len(t)) % 2 == 0, np.float32(0.35), np.float32(np.inf)).astype(np.float32)
    occ = np.zeros(len(t), np.int32)
    host.bvh_host_anyhit(_p(buf), _p(o), _p(d), C.c_long(len(t)), C.c_float(0.0), _p(t_max), _p(occ))
    assert np.array_equal(occ != 0, t_ref < t_max)


def test_standalone_program_under_sanitizers(tmp_path):
    """The stand-alone program (its own main, nothing loaded into Python) built with AddressSanitizer + UBSan, on the 320-triangle case."""
    exe = sanitized_program('dsdf_bvh_host.cpp')
    tri = MESHES['ico320']
    sets = ray_sets(tri, 6)
    o = np.concatenate([sets[k][0] for k in ('random', 'axis', 'inside', 'miss_root')])
    d = np.concatenate([sets[k][1] for k in ('random', 'axis', 'inside', 'miss_root')])
    fn = tmp_path / 'case.bin'
    with open(fn, 'wb') as fh:
        fh.write(np.asarray([tri.shape[0], o.shape[0]], np.int32).tobytes() + np.float32(0.0).tobytes())
        fh.write(tri.tobytes() + o.tobytes() + d.tobytes())
    run_case(exe, fn)
