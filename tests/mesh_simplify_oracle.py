"""TEST INFRASTRUCTURE ONLY -- fp64 numpy reference of the mesh simplification (csrc/dsdf_simplify.h: vertex clustering with quadric error
metrics), and the shared case table of its CPU and GPU tests.  Nothing under differentiable-sdf-rendering_amd/ imports it.

The cell of a vertex is taken in float32 with the kernel's statement (i = clamp(floor((v - lo) inv), 0, c - 1), inv = c / (hi - lo) in
float32): which cell a vertex on a boundary belongs to is a definition, not an approximation.  Everything else is fp64 and formulated
differently on purpose (a shared mistake must not hide): the kernel sums the quadric of a cell in coordinates relative to the cell's
centre, in sorted record order, and solves (A + lambda I) x = lambda m - b with a hand-written Cholesky factorisation; here the planes
are n . x + d0 = 0 in ABSOLUTE coordinates, the sums are vectorised over the cell's records, and the system goes through np.linalg.solve
(LU with pivoting).  The survivors are found from per-VERTEX cells (the kernel keys every face corner), the used cells by np.unique."""
import functools

import numpy as np

import mesh_closest_oracle as C
import mesh_oracle as M

REG = 1e-3
# max |x_fp32 - x_fp64| / cell size (per axis) of the HOST build of csrc/dsdf_simplify.h over every case of CASES below
# (`PYTHONPATH=oracle:tests python tests/test_mesh_simplify_host.py` prints it), and the gate of every comparison of positions, normals
# and colours with this reference: 4 x the measurement -- the factor covers other meshes and orders of summation, not other arithmetic.
MEASURED_MAX_ERR = 1.100e-05        # torus_9x9x5; sphere_6 1.075e-05, sheet_5 1.022e-05
GATE = 4 * MEASURED_MAX_ERR


def grid_of(lo, hi, cells):
    lo, hi = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    return lo, hi, np.asarray(cells, np.int64)


def vertex_cells(v, lo, hi, cells):
    """(V, 3) integer cell coordinates, binned in float32 with the kernel's statement."""
    lo, hi, c = grid_of(lo, hi, cells)
    inv = c.astype(np.float32) / (hi - lo)
    t = np.floor((np.asarray(v, np.float32) - lo) * inv)
    return np.clip(t, 0, (c - 1).astype(np.float32)).astype(np.int64)


def cell_keys(ijk, cells):
    return (ijk[:, 2] * cells[1] + ijk[:, 1]) * cells[0] + ijk[:, 0]


def cell_size(lo, hi, cells):
    lo, hi, c = grid_of(lo, hi, cells)
    return (hi.astype(np.float64) - lo.astype(np.float64)) / c


def diagonal(lo, hi, cells):
    return float(np.linalg.norm(cell_size(lo, hi, cells)))


def simplify(v, f, lo, hi, cells, reg=REG, colors=None):
    """-> dict: keys (F, 3) the cell key of every face corner; vertices (V', 3) fp64, faces (F', 3), normals (V', 3), colors (V', 3) or
    None, cell (V',) the key of every output vertex, mean (V', 3) the mean m of its corner records, clamped (V',) whether the clamp into
    the cell's box moved it, kept (F',) the input index of every output face."""
    v32 = np.asarray(v, np.float32)
    f = np.asarray(f, np.int64).reshape(-1, 3)
    lo32, hi32, c = grid_of(lo, hi, cells)
    x = v32.astype(np.float64)
    vkey = cell_keys(vertex_cells(v32, lo32, hi32, c), c)
    fkey = vkey[f] if len(f) else np.zeros((0, 3), np.int64)
    keep = (fkey[:, 0] != fkey[:, 1]) & (fkey[:, 1] != fkey[:, 2]) & (fkey[:, 2] != fkey[:, 0])
    used = np.unique(fkey[keep])
    faces = np.searchsorted(used, fkey[keep])
    size = cell_size(lo32, hi32, c)
    p = x[f]                                                      # (F, 3, 3)
    N = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]) if len(f) else np.zeros((0, 3))
    ln = np.linalg.norm(N, axis=1)
    ok = ln > 0
    n = np.where(ok[:, None], N / np.where(ok, ln, 1.0)[:, None], 0.0)
    a = np.where(ok, 0.5 * ln, 0.0)
    d0 = -(n * p[:, 0]).sum(1) if len(f) else np.zeros(0)
    pos, nrm, col, mean, clamped = (np.zeros((len(used), 3)) for _ in range(5))
    for r, key in enumerate(used):
        ff, kk = np.nonzero(fkey == key)                          # the cell's records: corner kk of face ff
        A = np.einsum('f,fi,fj->ij', a[ff], n[ff], n[ff])
        b = (a[ff] * d0[ff]) @ n[ff]
        area = a[ff].sum()
        m = x[f[ff, kk]].mean(0)
        if area > 0:
            lam = reg * area
            sol = np.linalg.solve(A + lam * np.eye(3), lam * m - b)
        else:
            sol = m
        ijk = np.asarray([key % c[0], (key // c[0]) % c[1], key // (c[0] * c[1])])
        blo = lo32.astype(np.float64) + ijk * size
        pos[r] = np.clip(sol, blo, blo + size)
        clamped[r] = pos[r] != sol
        mean[r] = m
        ns = 0.5 * N[ff].sum(0)
        nrm[r] = ns / np.linalg.norm(ns) if np.linalg.norm(ns) > 0 else 0.0
        if colors is not None:
            col[r] = np.asarray(colors, np.float64)[f[ff, kk]].mean(0)
    return dict(keys=fkey, vertices=pos, faces=faces, normals=nrm, colors=col if colors is not None else None, cell=used, mean=mean,
                clamped=clamped.any(1), kept=np.nonzero(keep)[0])


# ---- shared inputs ------------------------------------------------------------------------------------------------------------------
def cube(n=16, half=0.4, offset=(0.013, -0.007, 0.021)):
    """A cube of n x n quads per side with welded vertices and outward triangles."""
    ids, verts, faces = {}, [], []

    def vid(q):
        q = tuple(int(t) for t in q)
        if q not in ids:
            ids[q] = len(verts)
            verts.append(q)
        return ids[q]
    for axis in range(3):
        u, w = (axis + 1) % 3, (axis + 2) % 3
        for side in (0, n):
            for i in range(n):
                for j in range(n):
                    def q(di, dj):
                        t = [0, 0, 0]
                        t[axis], t[u], t[w] = side, i + di, j + dj
                        return vid(t)
                    a, b, c_, d = q(0, 0), q(1, 0), q(1, 1), q(0, 1)          # e_u x e_w = +e_axis
                    faces += [(a, b, c_), (a, c_, d)] if side else [(a, c_, b), (a, d, c_)]
    v = (np.asarray(verts, np.float64) / n * 2 - 1) * half + np.asarray(offset)
    return v.astype(np.float32), np.asarray(faces, np.int64)


def torus(nu=48, nv=24, R=0.3, r=0.1, centre=(0.004, -0.006, 0.003)):
    u, w = np.meshgrid(np.arange(nu) * 2 * np.pi / nu, np.arange(nv) * 2 * np.pi / nv, indexing='ij')
    v = np.stack([(R + r * np.cos(w)) * np.cos(u), (R + r * np.cos(w)) * np.sin(u), r * np.sin(w)], -1).reshape(-1, 3) + np.asarray(centre)
    faces = []
    for i in range(nu):
        for j in range(nv):
            a, b, c_, d = i * nv + j, ((i + 1) % nu) * nv + j, ((i + 1) % nu) * nv + (j + 1) % nv, i * nv + (j + 1) % nv
            faces += [(a, b, c_), (a, c_, d)]
    return v.astype(np.float32), np.asarray(faces, np.int64)


def sheet(n=12):
    """An open, gently curved sheet z = 0.1 sin(3 x) cos(2 y) over [-0.4, 0.4]^2."""
    t = np.linspace(-0.4, 0.4, n + 1)
    X, Y = np.meshgrid(t, t, indexing='ij')
    v = np.stack([X, Y, 0.1 * np.sin(3 * X) * np.cos(2 * Y) + 0.011], -1).reshape(-1, 3)
    faces = []
    for i in range(n):
        for j in range(n):
            a, b, c_, d = i * (n + 1) + j, (i + 1) * (n + 1) + j, (i + 1) * (n + 1) + j + 1, i * (n + 1) + j + 1
            faces += [(a, b, c_), (a, c_, d)]
    return v.astype(np.float32), np.asarray(faces, np.int64)


def flat(n=10):
    """A mesh in ONE plane (z = 0.0625 exactly), irregular in it: A has rank 1 in every cell."""
    rng = np.random.default_rng(3)
    t = np.linspace(-0.4, 0.4, n + 1)
    X, Y = np.meshgrid(t, t, indexing='ij')
    jit = rng.uniform(-0.02, 0.02, (2,) + X.shape)
    v = np.stack([X + jit[0], Y + jit[1], np.full_like(X, 0.0625)], -1).reshape(-1, 3)
    return v.astype(np.float32), sheet(n)[1]


def soup_to_indexed(tri, extra_vertex=None):
    """An indexed mesh of a triangle soup with equal corners welded (np.unique), plus an optional vertex that no face uses, in FRONT."""
    v, inv = np.unique(np.asarray(tri, np.float32).reshape(-1, 3), axis=0, return_inverse=True)
    f = inv.reshape(-1, 3).astype(np.int64)
    if extra_vertex is not None:
        v, f = np.concatenate([np.asarray([extra_vertex], np.float32), v]), f + 1
    return np.ascontiguousarray(v, np.float32), f


UNIT = ((-0.5, -0.5, -0.5), (0.5, 0.5, 0.5))
TORUS_BOX = ((-0.45, -0.45, -0.25), (0.45, 0.45, 0.25))
SPHERE_C, SPHERE_R = (0.021, -0.013, 0.017), 0.37
TWO = (((-0.1, 0.0, 0.0), 0.3), ((0.15, 0.05, 0.0), 0.25))


@functools.lru_cache(maxsize=None)
def mesh(name):
    if name == 'sphere':
        return M.icosphere(SPHERE_R, 3, centre=SPHERE_C)
    if name == 'cube':
        return cube()
    if name == 'torus':
        return torus()
    if name == 'two_spheres':
        (c0, r0), (c1, r1) = TWO
        (v0, f0), (v1, f1) = M.icosphere(r0, 2, centre=c0), M.icosphere(r1, 2, centre=c1)
        return np.concatenate([v0, v1]), np.concatenate([f0, f1 + len(v0)])
    if name == 'sheet':
        return sheet()
    if name == 'flat':
        return flat()
    if name == 'degenerate':
        return soup_to_indexed(C.MESHES['degenerate'], extra_vertex=(0.45, 0.45, 0.45))
    raise KeyError(name)


# name -> (mesh, (lo, hi), (cx, cy, cz)).  The first six are the prototype's runs.
CASES = {
    'sphere_6': ('sphere', UNIT, (6, 6, 6)), 'sphere_11': ('sphere', UNIT, (11, 11, 11)),
    'cube_5': ('cube', UNIT, (5, 5, 5)), 'cube_7': ('cube', UNIT, (7, 7, 7)),
    'torus_9x9x5': ('torus', TORUS_BOX, (9, 9, 5)), 'torus_4x4x2': ('torus', TORUS_BOX, (4, 4, 2)),
    'two_spheres_7': ('two_spheres', UNIT, (7, 7, 7)),
    'sheet_5': ('sheet', UNIT, (5, 5, 5)),
    'degenerate_3': ('degenerate', UNIT, (3, 3, 3)),
    'collapse_1': ('sphere', UNIT, (1, 1, 1)),
    'flat_4': ('flat', UNIT, (4, 4, 4)),
}
CLOSED = ('sphere_6', 'sphere_11', 'cube_5', 'cube_7', 'torus_9x9x5', 'torus_4x4x2', 'two_spheres_7')


def colors_of(v):
    """An affine colour field on the vertices (fp32): the mean colour of a cell is the field at the mean position."""
    x = np.asarray(v, np.float64)
    return np.stack([0.5 + 0.6 * x[:, 0], 0.5 - 0.4 * x[:, 1] + 0.3 * x[:, 2], 0.4 + 0.2 * x[:, 0] + 0.5 * x[:, 1]], -1).astype(np.float32)


def color_field(x):
    x = np.asarray(x, np.float64)
    return np.stack([0.5 + 0.6 * x[:, 0], 0.5 - 0.4 * x[:, 1] + 0.3 * x[:, 2], 0.4 + 0.2 * x[:, 0] + 0.5 * x[:, 1]], -1)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The fp64 result of a case with colours, computed once per process."""
    mname, (lo, hi), cells = CASES[name]
    v, f = mesh(mname)
    return simplify(v, f, lo, hi, cells, colors=colors_of(v))


def sample_surface(v, f, n, seed):
    """n area-weighted points on the triangles f of v (fp64)."""
    rng = np.random.default_rng(seed)
    t = np.asarray(v, np.float64)[np.asarray(f, np.int64)]
    area = 0.5 * np.linalg.norm(np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]), axis=1)
    pick = rng.choice(len(t), n, p=area / area.sum())
    s, w = np.sqrt(rng.uniform(size=n)), rng.uniform(size=n)
    a, b = s * (1 - w), s * w
    return t[pick, 0] + a[:, None] * (t[pick, 1] - t[pick, 0]) + b[:, None] * (t[pick, 2] - t[pick, 0])
