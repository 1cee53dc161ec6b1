"""TEST INFRASTRUCTURE ONLY -- plain-numpy reference of the mesh's connected components (csrc/dsdf_components.h; include/dsdf.h has the
definitions), and the shared case table of its CPU and GPU tests.  Nothing under differentiable-sdf-rendering_amd/ imports it.

Formulated differently from the kernels on purpose: a serial union-find with path halving that hooks by the ORDER OF ARRIVAL and takes
the minimum of every set afterwards (the kernels hook the larger root under the smaller one and never compress); the numbering through
np.unique (the binding scans a flag array); the measures in fp64 from numpy's cross / einsum; the boundary edges from a Python dict (the
binding sorts int64 edge keys)."""
import functools
import math

import numpy as np

import mesh_oracle as M
import mesh_simplify_oracle as S

# max over the case table and over both measures of |sum of the HOST build's fp32 terms - fp64 measure| / scale per component, the scale
# of an area being the area and that of a volume the sum of |p0| |p1| |p2| / 6 over its faces (volume_scale)
# (`PYTHONPATH=oracle:tests python tests/test_mesh_components_host.py` prints it), and the gate of the comparisons with the all-fp64
# measures: 4 x the measurement, as mesh_simplify_oracle.GATE was set.
MEASURED_MAX_ERR = 3.385e-06        # the area of a sliver among the random triangles of parts_20000; volumes 1.531e-07 (the same case)
GATE = 4 * MEASURED_MAX_ERR


def labels(faces, n_vertices):
    """label (V,) int32: the smallest vertex index of every vertex's component."""
    parent = list(range(n_vertices))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for a, b, c in np.asarray(faces, np.int64).reshape(-1, 3).tolist():
        for p, q in ((a, b), (b, c)):
            rp, rq = find(p), find(q)
            if rp != rq:
                parent[rq] = rp                                   # (no order: the minimum is taken below)
    root = np.asarray([find(v) for v in range(n_vertices)], np.int64)
    smallest = np.full(n_vertices, n_vertices, np.int64)
    np.minimum.at(smallest, root, np.arange(n_vertices))
    return smallest[root].astype(np.int32) if n_vertices else np.zeros(0, np.int32)


def numbering(label, faces):
    """-> (C, face_component (F,) int32, vertex_component (V,) int32): components in ascending order of their label, only those with a face."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    with_face = np.unique(label[faces[:, 0]]) if len(faces) else np.zeros(0, np.int32)
    fc = np.searchsorted(with_face, label[faces[:, 0]]).astype(np.int32) if len(faces) else np.zeros(0, np.int32)
    return len(with_face), fc, np.where(np.isin(label, with_face), np.searchsorted(with_face, label), -1).astype(np.int32)


def face_measures64(v, faces):
    """fp64 (area (F,), vol (F,)) of the float32 vertices."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    p = np.asarray(v, np.float64).reshape(-1, 3)[faces] if len(faces) else np.zeros((0, 3, 3))
    area = 0.5 * np.linalg.norm(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), axis=1)
    vol = np.einsum('fi,fi->f', p[:, 0], np.cross(p[:, 1], p[:, 2])) / 6.0
    return area, vol


def volume_scale(v, faces):
    """|p0| |p1| |p2| / 6 per face: what bounds every product of the triple product, hence the scale of its rounding error -- the term
    itself can be far smaller (a triangle seen edge-on from the origin), and an error relative to it would measure the cancellation."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    p = np.asarray(v, np.float64).reshape(-1, 3)[faces] if len(faces) else np.zeros((0, 3, 3))
    return np.linalg.norm(p, axis=2).prod(1) / 6.0


def exact_sums(terms, fc, C):
    """Per component: (the correctly rounded sum of `terms` as fp64 numbers (math.fsum), the sum of their magnitudes, the number of terms)."""
    terms = np.asarray(terms, np.float64)
    order = np.argsort(fc, kind='stable')
    ends = np.searchsorted(fc[order], np.arange(C + 1))
    s, a = np.zeros(C), np.zeros(C)
    for c in range(C):
        t = terms[order[ends[c]:ends[c + 1]]].tolist()
        s[c], a[c] = math.fsum(t), math.fsum(map(abs, t))
    return s, a, np.diff(ends)


def boundary_edges(faces, fc, C):
    """Per component the number of undirected edges that occur exactly once among the sides of the faces (a side between equal indices is
    none; the face (a, a, b) has the side a b twice, so that edge does not count)."""
    uses = {}
    for f, (a, b, c) in enumerate(np.asarray(faces, np.int64).reshape(-1, 3).tolist()):
        for p, q in ((a, b), (b, c), (c, a)):
            if p != q:
                uses.setdefault((min(p, q), max(p, q)), []).append(f)
    out = np.zeros(C, np.int64)
    for fs in uses.values():
        if len(fs) == 1:
            out[fc[fs[0]]] += 1
    return out


def bboxes(v, faces, fc, C):
    out = np.zeros((C, 2, 3), np.float32)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    for c in range(C):
        p = np.asarray(v, np.float32)[faces[fc == c].reshape(-1)]
        out[c, 0], out[c, 1] = p.min(0), p.max(0)
    return out


# ---- shared inputs ------------------------------------------------------------------------------------------------------------------
def _positions(n, seed):
    return np.random.default_rng(seed).uniform(-0.5, 0.5, (n, 3)).astype(np.float32)


def disjoint(n, shuffle_seed=None):
    """n triangles without a common vertex; with a seed the 3 n vertex numbers are shuffled."""
    f = np.arange(3 * n, dtype=np.int64).reshape(n, 3)
    if shuffle_seed is not None:
        f = np.random.default_rng(shuffle_seed).permutation(3 * n)[f]
    return _positions(3 * n, n), f


def strip(n):
    """One triangle strip of n faces over n + 2 vertices."""
    i = np.arange(n, dtype=np.int64)
    f = np.stack([i, i + 1, i + 2], -1)
    f[1::2] = f[1::2][:, [1, 0, 2]]
    x = np.arange(n + 2)
    return np.stack([0.01 * (x // 2), 0.01 * (x % 2), 0.002 * np.sin(0.3 * x)], -1).astype(np.float32), f


def ribbon(n, order):
    """n quads in a row, 2 n + 2 vertices; `order`: 'asc' numbers the vertices along the ribbon, 'desc' against it, an int = a seeded
    permutation.  The same surface each time."""
    j = np.arange(n, dtype=np.int64)
    a, b, c, d = 2 * j, 2 * j + 1, 2 * j + 3, 2 * j + 2
    f = np.stack([np.stack([a, b, c], -1), np.stack([a, c, d], -1)], 1).reshape(-1, 3)
    x = np.arange(2 * n + 2)
    v = np.stack([(x // 2) / n - 0.5, 0.02 * (x % 2), 0.05 * np.sin(40.0 * (x // 2) / n)], -1).astype(np.float32)
    V = 2 * n + 2
    new = np.arange(V) if order == 'asc' else (V - 1 - np.arange(V) if order == 'desc' else np.random.default_rng(order).permutation(V))
    vv = np.empty_like(v)
    vv[new] = v
    return vv, new[f]


def fan(n, hub_last):
    """n triangles round one hub vertex (the rim is open: n + 1 rim vertices); the hub is vertex 0 or vertex V - 1."""
    t = np.arange(n + 1) * (2 * np.pi / (n + 1))
    rim = np.stack([0.4 * np.cos(t), 0.4 * np.sin(t), 0.01 * np.sin(7 * t)], -1)
    j = np.arange(n, dtype=np.int64)
    if hub_last:
        v, f = np.concatenate([rim, [[0.0, 0.0, 0.1]]]), np.stack([np.full(n, n + 1), j, j + 1], -1)
    else:
        v, f = np.concatenate([[[0.0, 0.0, 0.1]], rim]), np.stack([np.zeros(n, np.int64), j + 1, j + 2], -1)
    return v.astype(np.float32), f


def unreferenced():
    """Two triangles with vertices that no face names in front of, between and behind them."""
    return _positions(11, 5), np.asarray([[2, 3, 4], [7, 9, 8]], np.int64)


SPHERES_SUBDIV = 4        # volume / (4 pi r^3 / 3) of an icosphere: 0.9662 at subdivision 2 (the simplify table's), 0.9914 at 3, 0.9978 at 4


@functools.lru_cache(maxsize=None)
def mesh(name):
    """(vertices (V, 3) float32, faces (F, 3) int64) of one case."""
    small = {'one_triangle': [[0, 1, 2]], 'shared_edge': [[0, 1, 2], [2, 1, 3]], 'shared_vertex': [[0, 1, 2], [2, 3, 4]],
             'two_disjoint': [[0, 1, 2], [3, 4, 5]], 'repeated_index': [[1, 1, 3], [0, 2, 2]]}
    if name in small:
        f = np.asarray(small[name], np.int64)
        return _positions(int(f.max()) + 1, len(name)), f
    if name == 'empty_0':
        return np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64)
    if name == 'empty_5':
        return _positions(5, 1), np.zeros((0, 3), np.int64)
    if name == 'unreferenced':
        return unreferenced()
    kind, _, arg = name.partition('_')
    if kind == 'disjoint':
        return disjoint(int(arg))
    if kind == 'strip':
        return strip(int(arg))
    if kind == 'ribbon':
        return ribbon(4096, arg if arg in ('asc', 'desc') else 11)
    if kind == 'fan':
        return fan(10000, arg == 'hublast')
    if name == 'parts_20000':
        return disjoint(20000, shuffle_seed=3)
    if name == 'two_spheres':
        (c0, r0), (c1, r1) = S.TWO
        (v0, f0), (v1, f1) = M.icosphere(r0, SPHERES_SUBDIV, centre=c0), M.icosphere(r1, SPHERES_SUBDIV, centre=c1)
        return np.concatenate([v0, v1]), np.concatenate([f0, f1 + len(v0)])
    if name == 'sphere_soup':                                    # every face with three vertices of its own
        v, f = S.mesh('sphere')
        return np.ascontiguousarray(v[f].reshape(-1, 3)), np.arange(3 * len(f), dtype=np.int64).reshape(-1, 3)
    return S.mesh(name)                                          # torus, sheet


CASES = ('empty_0', 'empty_5', 'one_triangle', 'shared_edge', 'shared_vertex', 'two_disjoint', 'repeated_index', 'unreferenced',
         'disjoint_255', 'disjoint_256', 'disjoint_257', 'strip_255', 'strip_256', 'strip_257', 'ribbon_asc', 'ribbon_desc', 'ribbon_perm',
         'fan_hub0', 'fan_hublast', 'parts_20000', 'two_spheres', 'torus', 'sheet', 'sphere_soup')
DEGENERATE = ('empty_0', 'empty_5', 'one_triangle', 'shared_edge', 'shared_vertex', 'two_disjoint', 'repeated_index', 'unreferenced')
# what is known without computing anything: name -> (C, components without a boundary edge; the two faces (a, a, b) of repeated_index
# have none: their one edge occurs twice)
KNOWN = {'empty_0': (0, 0), 'empty_5': (0, 0), 'one_triangle': (1, 0), 'shared_edge': (1, 0), 'shared_vertex': (1, 0), 'two_disjoint': (2, 0),
         'repeated_index': (2, 2), 'unreferenced': (2, 0), 'disjoint_255': (255, 0), 'disjoint_256': (256, 0), 'disjoint_257': (257, 0),
         'strip_255': (1, 0), 'strip_256': (1, 0), 'strip_257': (1, 0), 'ribbon_asc': (1, 0), 'ribbon_desc': (1, 0), 'ribbon_perm': (1, 0),
         'fan_hub0': (1, 0), 'fan_hublast': (1, 0), 'parts_20000': (20000, 0), 'two_spheres': (2, 2), 'torus': (1, 1), 'sheet': (1, 0),
         'sphere_soup': (1280, 0)}


@functools.lru_cache(maxsize=None)
def reference(name):
    """Everything the definitions give for one case, computed once per process and never changed: label, n, face_component,
    vertex_component, faces_per_component, area / volume (fp64 sums of fp64 terms), abs_area / abs_volume (the scales an error of
    them is relative to: the area itself, the sum of volume_scale), bbox, boundary_edges."""
    v, f = mesh(name)
    lab = labels(f, len(v))
    C, fc, vc = numbering(lab, f)
    a64, w64 = face_measures64(v, f)
    area, abs_area, count = exact_sums(a64, fc, C)
    volume = exact_sums(w64, fc, C)[0]
    abs_volume = exact_sums(volume_scale(v, f), fc, C)[0]
    out = dict(label=lab, n=C, face_component=fc, vertex_component=vc, faces_per_component=count.astype(np.int64), area=area, volume=volume,
               abs_area=abs_area, abs_volume=abs_volume, bbox=bboxes(v, f, fc, C), boundary_edges=boundary_edges(f, fc, C))
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out
