"""TEST INFRASTRUCTURE ONLY -- the numpy oracle of the surface extraction (csrc/dsdf_iso.h, include/dsdf.h: dsdf_iso_*), written from
the specification, not from the kernel, and the cases the host and the GPU tests share.

Specification.  Lattice of nx x ny x nz cells over the unit cube, nodes (i/nx, j/ny, k/nz), node index (k (ny + 1) + j)(nx + 1) + i; a
node is inside iff values[node] < iso.  A node owns the edges towards its upper neighbours (types 0 +x, 1 +y, 2 +z, 3 +x+y, 4 +x+z,
5 +y+z, 6 +x+y+z); an edge with exactly one inside end carries one vertex; vertices ordered by owning node, then type.  Every cell is
cut into the six Kuhn tetrahedra c, c + e_a, c + e_a + e_b, c + (1,1,1) of the axis orders xyz, xzy, yxz, yzx, zxy, zyx; with I / O the
inside / outside corners of a tetrahedron (ascending) and e(p, q) the vertex on edge vp vq:
    |I| = 1: e(a,O0) e(a,O1) e(a,O2);   |I| = 3: e(I0,d) e(I1,d) e(I2,d);   |I| = 2: q0 q1 q2, q0 q2 q3 of q = e(a,c) e(a,d) e(b,d) e(b,c)
each triangle oriented (swap of its last two vertices) so that (B - A) x (C - A) points from the inside corners to the outside ones.
Faces ordered by cell, tetrahedron, listing.  Vertex position: bisection on the edge from the bracket the node signs give."""
import numpy as np
import torch

import sdf_oracle as O

EDGE_TYPES = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [1, 0, 1], [0, 1, 1], [1, 1, 1]])      # (dx, dy, dz) of type t
TET_ORDERS = ('xyz', 'xzy', 'yxz', 'yzx', 'zxy', 'zyx')
_AXIS = {'x': 0, 'y': 1, 'z': 2}


# (c) |f64(vertex) - iso| of the vertices the host build (tests/test_iso_host.py) places, f64 = the fp64 oracle's lookup: the largest value over sphere16,
# blob32 and blob32_24 at the grid's own resolution, 24 steps, is 1.03e-7 (sphere16; blob32 8.0e-8, blob32_24 9.2e-8) -- fp32 noise of
# the lookup, the bisection itself reaches 1e-13 in fp64.  Gate = 4 x that; the margin covers the device contracting FMAs differently.
VERTEX_RESIDUAL_MEASURED = 1.03e-7
VERTEX_RESIDUAL_GATE = 4 * VERTEX_RESIDUAL_MEASURED
# A stored position is a + s (b - a) after three fp32 roundings of numbers below 1 (the node i / n, the difference, the fused
# multiply-add), each at most 2^-24: it lies within sqrt(3) * 3 * 2^-24 of the exact segment.
ON_EDGE_TOL = 3 ** 0.5 * 3 * 2.0 ** -24


def tet_corners(tet):
    """(4, 3) integer corner offsets (x, y, z) of tetrahedron `tet` from the lower cell corner."""
    c = [np.zeros(3, np.int64)]
    for ch in TET_ORDERS[tet]:
        v = c[-1].copy()
        v[_AXIS[ch]] = 1
        c.append(v)
    return np.stack(c)


def case_triangles(mask):
    """The triangles of a sign case (bit p of mask: corner vp is inside) as triples of corner pairs, before orientation."""
    I = [p for p in range(4) if (mask >> p) & 1]
    Out = [p for p in range(4) if not (mask >> p) & 1]
    if len(I) == 1:
        return [[(I[0], Out[0]), (I[0], Out[1]), (I[0], Out[2])]]
    if len(I) == 3:
        return [[(I[0], Out[0]), (I[1], Out[0]), (I[2], Out[0])]]
    if len(I) == 2:
        (a, b), (c, d) = I, Out
        q = [(a, c), (a, d), (b, d), (b, c)]
        return [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]
    return []


def needs_swap(tet, mask, tri, s=None):
    """The geometric rule: with the vertices at parameter s[(p, q)] (default: the middle) of their edges, does (B - A) x (C - A) point
    from the outside corners to the inside ones?"""
    v = tet_corners(tet).astype(np.float64)
    I = [p for p in range(4) if (mask >> p) & 1]
    Out = [p for p in range(4) if not (mask >> p) & 1]
    towards_outside = v[Out].mean(0) - v[I].mean(0)

    def pos(e):
        p, q = min(e), max(e)
        t = 0.5 if s is None else s[(p, q)]
        return v[p] + t * (v[q] - v[p])
    A, B, C = (pos(e) for e in tri)
    return float(np.cross(B - A, C - A) @ towards_outside) < 0.0


def oriented_case_table():
    """[tet][mask] -> list of triangles (triples of (p, q) corner pairs, p < q), oriented by the geometric rule."""
    tab = []
    for tet in range(6):
        row = []
        for mask in range(16):
            tris = []
            for tri in case_triangles(mask):
                tri = [(min(e), max(e)) for e in tri]
                if needs_swap(tet, mask, tri):
                    tri = [tri[0], tri[2], tri[1]]
                tris.append(tri)
            row.append(tris)
        tab.append(row)
    return tab


_TABLE = oriented_case_table()


def n_nodes(n):
    nx, ny, nz = n
    return (nx + 1) * (ny + 1) * (nz + 1)


def node_positions(n):
    """(N, 3) float64 node positions (x, y, z) in node-index order."""
    nx, ny, nz = n
    k, j, i = np.meshgrid(np.arange(nz + 1), np.arange(ny + 1), np.arange(nx + 1), indexing='ij')
    return np.stack([i.reshape(-1) / nx, j.reshape(-1) / ny, k.reshape(-1) / nz], -1)


def topology(values, n, iso=0.0):
    """The exact outputs of dsdf_iso_mark + dsdf_iso_emit for the buffer `values` (N,), compared in ITS dtype against iso in that dtype:
    dict(cross (N,) uint8, n_vert (N,) int32, n_tri (N,) int32, vert_edge (V,) int32, faces (F, 3) int32, tet_case (F, 2): the
    (tetrahedron, case) every face came from)."""
    nx, ny, nz = n
    values = np.asarray(values)
    N = n_nodes(n)
    assert values.shape == (N,)
    inside = (values < values.dtype.type(iso)).reshape(nz + 1, ny + 1, nx + 1)
    sx, sxy = nx + 1, (nx + 1) * (ny + 1)
    crossing = np.zeros((nz + 1, ny + 1, nx + 1, 7), bool)
    for t, (dx, dy, dz) in enumerate(EDGE_TYPES):
        a = inside[:nz + 1 - dz, :ny + 1 - dy, :nx + 1 - dx]
        b = inside[dz:, dy:, dx:]
        crossing[:nz + 1 - dz, :ny + 1 - dy, :nx + 1 - dx, t] = a != b
    crossing = crossing.reshape(N, 7)
    cross = (crossing * (1 << np.arange(7))).sum(1).astype(np.uint8)
    n_vert = crossing.sum(1).astype(np.int32)
    node, typ = np.nonzero(crossing)                                          # row-major: by node, then type
    vert_edge = (8 * node + typ).astype(np.int32)
    vid = np.full(8 * N, -1, np.int64)
    vid[vert_edge] = np.arange(vert_edge.size)
    # cells
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing='ij')
    cell = ((k * (ny + 1) + j) * (nx + 1) + i).reshape(-1)
    rows = []                                                                 # (cell node, tet, listing index, v0, v1, v2, case)
    for tet in range(6):
        corners = tet_corners(tet)
        off = corners[:, 0] + corners[:, 1] * sx + corners[:, 2] * sxy           # node offset of each tetrahedron corner
        ins = inside.reshape(-1)[cell[:, None] + off[None, :]]                  # (cells, 4)
        mask = (ins * (1 << np.arange(4))).sum(1)
        for m in range(1, 15):
            sel = cell[mask == m]
            if sel.size == 0:
                continue
            for idx, tri in enumerate(_TABLE[tet][m]):
                ids = []
                for p, q in tri:
                    d = corners[q] - corners[p]
                    t = int(np.nonzero((EDGE_TYPES == d).all(1))[0][0])
                    ids.append(vid[8 * (sel + off[p]) + t])
                rows.append(np.stack([sel, np.full(sel.size, tet), np.full(sel.size, idx)] + ids + [np.full(sel.size, m)], 1))
    if rows:
        rows = np.concatenate(rows)
        rows = rows[np.lexsort((rows[:, 2], rows[:, 1], rows[:, 0]))]
    else:
        rows = np.zeros((0, 7), np.int64)
    assert (rows[:, 3:6] >= 0).all()
    n_tri = np.bincount(rows[:, 0], minlength=N).astype(np.int32)
    return dict(cross=cross, n_vert=n_vert, n_tri=n_tri, vert_edge=vert_edge, faces=rows[:, 3:6].astype(np.int32), tet_case=rows[:, [1, 6]])


def canonical_faces(faces):
    """Every face rotated so that its smallest vertex id comes first (faces are compared up to cyclic rotation)."""
    f = np.asarray(faces).reshape(-1, 3)
    r = f.argmin(1)
    return np.stack([f[np.arange(len(f)), (r + s) % 3] for s in range(3)], 1)


def assert_same_topology(got, ref, what):
    for k in ('cross', 'n_vert', 'n_tri', 'vert_edge'):
        assert np.array_equal(got[k], ref[k]), (what, k)
    assert got['faces'].shape == ref['faces'].shape, what
    assert np.array_equal(canonical_faces(got['faces']), canonical_faces(ref['faces'])), (what, 'faces')


def edge_endpoints(vert_edge, n):
    """(a, b): float64 positions (V, 3) of the owning and the far node of every vertex's edge, and the owning node index."""
    nx, ny, nz = n
    ve = np.asarray(vert_edge, np.int64)
    node, typ = ve >> 3, ve & 7
    i = node % (nx + 1); j = (node // (nx + 1)) % (ny + 1); k = node // ((nx + 1) * (ny + 1))
    ijk = np.stack([i, j, k], -1)
    res = np.array([nx, ny, nz], np.float64)
    return ijk / res, (ijk + EDGE_TYPES[typ]) / res, node


def f64(data, pts, order=0):
    """The fp64 oracle's tricubic lookup at (n, 3) points of the cube: v, or (v, g)."""
    v, g, _ = O.eval_cubic(torch.as_tensor(np.asarray(data, np.float64)), torch.as_tensor(np.asarray(pts, np.float64)), order)
    return v.numpy() if order == 0 else (v.numpy(), g.numpy())


def oracle_values(data, n):
    return f64(data, node_positions(n))


def oracle_mesh(data, n, iso=0.0, steps=48):
    """The whole extraction in fp64: dict(values, topology..., positions (V, 3), normals (V, 3))."""
    values = oracle_values(data, n)
    topo = topology(values, n, iso)
    a, b, node = edge_endpoints(topo['vert_edge'], n)
    inside_a = values[node] < iso
    s0 = np.zeros(len(node)); s1 = np.ones(len(node))
    for _ in range(steps):
        sm = 0.5 * (s0 + s1)
        same = (f64(data, a + sm[:, None] * (b - a)) < iso) == inside_a
        s0 = np.where(same, sm, s0); s1 = np.where(same, s1, sm)
    pos = a + (0.5 * (s0 + s1))[:, None] * (b - a)
    if len(node):
        _, g = f64(data, pos, 1)
        nrm = g / np.linalg.norm(g, axis=1, keepdims=True)
    else:
        nrm = np.zeros((0, 3))
    return dict(topo, values=values, positions=pos, normals=nrm)


def manifold_report(faces, n_vertices):
    """closed: every directed edge occurs once and its reverse once; euler = V - E + F over the vertices the faces use."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    de = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    key = de[:, 0] * (n_vertices + 1) + de[:, 1]
    rkey = de[:, 1] * (n_vertices + 1) + de[:, 0]
    uniq, cnt = np.unique(key, return_counts=True)
    closed = bool((cnt == 1).all() and np.isin(rkey, uniq).all())
    und = np.unique(np.sort(de, 1), axis=0)
    V = np.unique(f).size
    return dict(closed=closed, euler=int(V - len(und) + len(f)), edges=len(und))


def border_inside(values, n, iso=0.0):
    """Does an inside node lie on the lattice border (where the mesh stays open)?"""
    nx, ny, nz = n
    ins = (np.asarray(values) < iso).reshape(nz + 1, ny + 1, nx + 1)
    inner = np.zeros_like(ins)
    inner[1:-1, 1:-1, 1:-1] = True
    return bool((ins & ~inner).any())


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
def _single(n, at):
    nx, ny, nz = n
    v = np.ones((nz + 1, ny + 1, nx + 1), np.float32)
    v[at[2], at[1], at[0]] = -1.0
    return v.reshape(-1)


def value_lattices():
    """name -> (n = (nx, ny, nz), values (N,) float32): lattices of values uploaded as they are."""
    rng = np.random.default_rng(0)
    n = (5, 4, 3)
    out = {
        'random_5x4x3': (n, rng.uniform(-1.0, 1.0, n_nodes(n)).astype(np.float32)),
        'zeros_5x4x3': (n, rng.choice(np.array([-1.0, 0.0, 1.0], np.float32), n_nodes(n))),
        'one_inside_2x2x2': ((2, 2, 2), _single((2, 2, 2), (1, 1, 1))),
        'one_on_border_2x2x2': ((2, 2, 2), _single((2, 2, 2), (2, 1, 1))),
        'single_cell': ((1, 1, 1), np.array([0.5, -0.25, 0.75, -1.0, 0.125, 0.5, -0.5, 0.25], np.float32)),
    }
    return out


VALUE_LATTICES = value_lattices()

_grids = {}


def grid(name):
    """The fp64 grids of the extraction tests (built once)."""
    if name not in _grids:
        _grids[name] = {'sphere16': lambda: O.sphere_grid(16), 'blob32': lambda: O.blob_grid(32, n=6, seed=1),
                        'blob32_24': lambda: O.blob_grid(32)}[name]().numpy()
    return _grids[name]


GRID_CASES = {'sphere16': (16, 16, 16), 'blob32': (32, 32, 32), 'blob32_24': (32, 32, 32)}

_oracle_meshes = {}


def oracle_mesh_of(name, n):
    key = (name, tuple(n))
    if key not in _oracle_meshes:
        _oracle_meshes[key] = oracle_mesh(grid(name), tuple(n))
    return _oracle_meshes[key]
