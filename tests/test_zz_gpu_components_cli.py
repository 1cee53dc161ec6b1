"""The command lines of the mesh's connected components as child processes on the GPU: `mesh_components.py`, `extract_mesh.py
--keep-largest` and `mesh_distance.py --largest-component` on a tiny SDF checkpoint with two blobs, the small one clearly apart from the
large one -- the floater an optimisation leaves.  The written files hold one component, and the printed counts match."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import iso_cases as I

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PY = os.path.join(ROOT, 'differentiable-sdf-rendering_amd', 'python')
RES = 32
# five lattice cells of empty space between them; the nodes where the small sphere is the nearer one (x > 0.735) lie beyond the four-node
# stencil of every lookup on the large sphere's surface (x <= 0.65 + 2 / 31), so the large sphere is extracted as it is alone
BIG, SMALL = ((0.4, 0.5, 0.5), 0.25), ((0.88, 0.5, 0.5), 0.06)
# sphere_grid puts node i at i / (RES - 1); the lookup the mesh is extracted from reads it as the texel centre (i + 0.5) / RES: the sphere
# it sees is smaller by (RES - 1) / RES and shifted accordingly
SEEN_R = BIG[1] * (RES - 1) / RES
SEEN_C = (np.asarray(BIG[0]) * (RES - 1) + 0.5) / RES


@pytest.fixture(scope='module')
def dsdf(built):
    import dsdf as m
    m.load()
    return m


@pytest.fixture()
def two_blobs(tmp_path):
    """sdf.vol: min of two sphere distances on the lattice of iso_cases' sphere grids; big.vol: the large sphere alone."""
    import util
    big, small = (I.O.sphere_grid(RES, c, r).float() for c, r in (BIG, SMALL))
    util.write_vol(str(tmp_path / 'sdf.vol'), torch.minimum(big, small))
    util.write_vol(str(tmp_path / 'big.vol'), big)
    return str(tmp_path / 'sdf.vol'), str(tmp_path / 'big.vol')


def run(script, *args):
    r = subprocess.run([sys.executable, os.path.join(PY, script)] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout
    return r.stdout


def components_of(dsdf, fn):
    import mesh_to_sdf
    v, f = mesh_to_sdf.load_mesh_indexed(fn)
    comp = dsdf.mesh_components(torch.from_numpy(np.ascontiguousarray(f).astype(np.int32)).cuda(), vertices=torch.from_numpy(np.ascontiguousarray(v, np.float32)).cuda())
    return comp, len(f)


def test_extract_mesh_keep_largest(dsdf, two_blobs, tmp_path):
    sdf, big = two_blobs
    everything, largest, alone = (str(tmp_path / n) for n in ('all.ply', 'largest.ply', 'alone.ply'))
    run('extract_mesh.py', sdf, '-o', everything)
    out = run('extract_mesh.py', sdf, '--keep-largest', '-o', largest)
    run('extract_mesh.py', big, '-o', alone)
    m = re.search(r'components: (\d+) found, (\d+) kept, (\d+) -> (\d+) faces', out)
    assert m, out
    found, kept, before, after = (int(g) for g in m.groups())
    both, n_all = components_of(dsdf, everything)
    one, n_largest = components_of(dsdf, largest)
    assert both.n == 2 == found and one.n == 1 == kept and (before, after) == (n_all, n_largest) and after < before
    assert both.boundary_edges.tolist() == [0, 0] and one.boundary_edges.tolist() == [0]
    assert after == int(both.faces_per_component.max()) and abs(float(one.area[0]) / float(both.area.max()) - 1.0) < 1e-12
    # the large sphere's surface: its area to the few per cent of a 32^3 lattice, and as many faces as the sphere extracted alone
    print(f'area of the large sphere {float(one.area[0]):.6f}, 4 pi r^2 = {4 * np.pi * SEEN_R ** 2:.6f}')
    assert abs(float(one.area[0]) / (4 * np.pi * SEEN_R ** 2) - 1.0) < 0.05
    assert components_of(dsdf, alone)[1] == after
    # the area threshold alone does the same here; both filters and a simplification go together
    out = run('extract_mesh.py', sdf, '--min-component-area', float(both.area.min()) * 1.5, '-o', largest)
    assert f'components: 2 found, 1 kept, {before} -> {after} faces' in out
    out = run('extract_mesh.py', sdf, '--keep-largest', '2', '--min-component-area', '1e-6', '--simplify', '8', '-o', largest)
    assert f'components: 2 found, 2 kept, {before} -> {before} faces' in out and 'simplified at 8 cells' in out


def test_mesh_components_cli(dsdf, two_blobs, tmp_path):
    sdf, big = two_blobs
    listing, out_ply, out_obj = (str(tmp_path / n) for n in ('list.json', 'out.ply', 'out.obj'))
    out = run('mesh_components.py', sdf, '--json', listing)
    assert '2 components' in out and out.count(', closed,') == 2 and 'boundary edges)' not in out
    rows = json.load(open(listing))['components']
    assert len(rows) == 2 and all(r['closed'] and r['boundary_edges'] == 0 for r in rows)
    big_row = max(rows, key=lambda r: r['area'])
    print(f'volume of the large sphere {big_row["volume"]:.6f}, 4 pi r^3 / 3 = {4 * np.pi * SEEN_R ** 3 / 3:.6f}')
    assert abs(big_row['volume'] / (4 * np.pi * SEEN_R ** 3 / 3) - 1.0) < 0.05 and big_row['faces'] > min(r['faces'] for r in rows)
    lo, hi = np.asarray(big_row['bbox'])
    assert np.abs(lo - (SEEN_C - SEEN_R)).max() < 0.5 / RES and np.abs(hi - (SEEN_C + SEEN_R)).max() < 0.5 / RES
    # the same from a mesh file, filtered and written in both formats
    everything = str(tmp_path / 'all.ply')
    run('extract_mesh.py', sdf, '-o', everything)
    for dst in (out_ply, out_obj):
        out = run('mesh_components.py', everything, '-o', dst, '--keep-largest', '1')
        m = re.search(r'components: 2 found, 1 kept, (\d+) -> (\d+) faces', out)
        assert m, out
        comp, n_faces = components_of(dsdf, dst)
        assert comp.n == 1 and n_faces == int(m.group(2)) == big_row['faces'] and comp.boundary_edges.tolist() == [0]
    out = run('mesh_components.py', everything, '-o', out_ply, '--min-faces', big_row['faces'] + 1)
    assert f'components: 2 found, 0 kept, {m.group(1)} -> 0 faces' in out and '0 vertices, 0 faces' in out


def test_mesh_distance_largest_component(two_blobs, tmp_path):
    """Against the large sphere alone the two-blob grid is far off where the floater is; with --largest-component it is the same surface."""
    sdf, big = two_blobs
    with_floater, without = (str(tmp_path / n) for n in ('a.json', 'b.json'))
    run('mesh_distance.py', sdf, big, '--samples', '20000', '--json', with_floater)
    run('mesh_distance.py', sdf, big, '--samples', '20000', '--largest-component', '--json', without)
    a, b = json.load(open(with_floater)), json.load(open(without))
    assert a['a_to_b_max'] > 0.15                     # the floater's far side: about 0.93 - 0.65
    assert b['a_to_b_max'] < 1e-5 and b['b_to_a_max'] < 1e-6 and b['hausdorff'] < a['hausdorff']
