"""Shared inputs of the mesh BVH tests (CPU and GPU): a numpy builder that writes the buffer from the layout documented in
include/dsdf.h, the mesh shapes and the ray sets."""
import numpy as np

import mesh_oracle as M

MARGIN = np.float32(2.0 ** -13)


# ---- numpy builder: include/dsdf.h's layout, nothing else ------------------------------------------------------------------
def n_leaves(T):
    L = 1
    while L < (T + 3) // 4:
        L *= 2
    return L


def morton_order(tri):
    c = tri.reshape(-1, 3, 3).mean(1)
    lo, hi = tri.reshape(-1, 3).min(0), tri.reshape(-1, 3).max(0)
    ext = np.where(hi > lo, hi - lo, 1.0)
    q = np.clip(((c - lo) / ext * 1024).astype(np.int64), 0, 1023)
    code = np.zeros(len(c), np.int64)
    for b in range(10):
        for a in range(3):
            code |= ((q[:, a] >> b) & 1) << (3 * b + 2 - a)
    return np.argsort(code, kind='stable').astype(np.int32)


def numpy_bvh(tri, order=None, normals=None):
    tri = np.ascontiguousarray(tri, np.float32).reshape(-1, 3, 3)
    T = tri.shape[0]
    L = n_leaves(T)
    order = np.arange(T, dtype=np.int32) if order is None else np.asarray(order, np.int32)
    buf = np.zeros(L * (100 if normals is not None else 64), np.float32)
    ints = buf.view(np.int32)
    pts = tri.reshape(-1, 3)
    lo, hi = pts.min(0), pts.max(0)
    margin = np.float32(MARGIN * (hi - lo).max())
    ints[0], ints[1], ints[2] = T, L, int(normals is not None)
    buf[3] = margin
    buf[4:7], buf[7:10] = lo, hi
    slots = buf[16 * L:64 * L].reshape(4 * L, 12)
    slots.view(np.int32)[:, 9] = -1
    slots[:T, :9] = tri[order].reshape(T, 9)
    slots.view(np.int32)[:T, 9] = order
    if normals is not None:
        buf[64 * L:100 * L].reshape(4 * L, 9)[:T] = np.asarray(normals, np.float32).reshape(-1, 9)[order]
    # boxes of all 2 L - 1 heap nodes, bottom-up; empty = inverted
    blo = np.full((2 * L - 1, 3), np.inf, np.float32)
    bhi = np.full((2 * L - 1, 3), -np.inf, np.float32)
    st = tri[order]
    e1, e2 = st[:, 1] - st[:, 0], st[:, 2] - st[:, 0]
    cr = np.cross(e1, e2)
    with np.errstate(over='ignore', invalid='ignore'):
        degenerate = ~((cr * cr).sum(1) > np.float32(2.0 ** -20) * (e1 * e1).sum(1) * (e2 * e2).sum(1))
    tlo = np.where(degenerate[:, None], -np.inf, st.min(1) - margin).astype(np.float32)
    thi = np.where(degenerate[:, None], np.inf, st.max(1) + margin).astype(np.float32)
    for s in range(T):
        j = L - 1 + s // 4
        blo[j] = np.minimum(blo[j], tlo[s]); bhi[j] = np.maximum(bhi[j], thi[s])
    for i in range(L - 2, -1, -1):
        blo[i] = np.minimum(blo[2 * i + 1], blo[2 * i + 2]); bhi[i] = np.maximum(bhi[2 * i + 1], bhi[2 * i + 2])
    nodes = buf[16:16 * L].reshape(L - 1, 16)
    for i in range(1, 2 * L - 1):
        nodes[(i - 1) // 2, 6 * ((i - 1) & 1):6 * ((i - 1) & 1) + 6] = np.concatenate([blo[i], bhi[i]])
    return buf


# ---- meshes -------------------------------------------------------------------------------------------------------------------
def meshes():
    out = {}
    box = (lambda vf: vf[0][vf[1]])(M.box())
    out['T1'] = box[:1]
    out['T4'] = box[:4]
    out['T5'] = box[:5]
    out['box12'] = box
    for s, name in ((2, 'ico320'), (4, 'ico5120')):
        v, f = M.icosphere(0.3, s, centre=(0.05, -0.02, 0.01))
        out[name] = v[f]
    v, f = M.icosphere(0.3, 1)
    ico = v[f]
    out['duplicated'] = np.concatenate([ico, ico[::-1], ico[:7]])            # equal t, equal Morton codes
    deg = np.stack([np.stack([box[0, 0], box[0, 0], box[0, 2]]),             # p0 == p1
                    np.stack([box[3, 0], box[3, 1], box[3, 1]]),             # p1 == p2: e1 == e2, a determinant of rounding noise
                    np.stack([box[5, 1]] * 3),                               # a point
                    np.asarray([[-0.2, -0.1, 0.0], [0.0, 0.05, 0.1], [0.2, 0.2, 0.2]], np.float32)])   # three distinct collinear corners
    out['zero_area'] = np.concatenate([box[:6], deg, box[6:]])
    g = np.linspace(-0.3, 0.3, 6, dtype=np.float32)
    quads = []
    for a in range(5):
        for b in range(5):
            p = [np.asarray([g[a + i], g[b + j], 0.125], np.float32) for i, j in ((0, 0), (1, 0), (1, 1), (0, 1))]
            quads += [np.stack([p[0], p[1], p[2]]), np.stack([p[0], p[2], p[3]])]
    out['coplanar'] = np.stack(quads)                                       # zero-thickness boxes
    return {k: np.ascontiguousarray(v, np.float32) for k, v in out.items()}


def ray_sets(tri, seed):
    rng = np.random.default_rng(seed)
    unit = lambda n: (lambda d: (d / np.linalg.norm(d, axis=1, keepdims=True)))(rng.normal(size=(n, 3)))
    sets = {}
    sets['random'] = (rng.uniform(-0.5, 0.5, (1000, 3)), unit(1000), 0.0)
    vc = M.voxel_centres(8)                                                  # includes origins on the symmetry planes of the meshes
    axes = np.asarray([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float64)
    sets['axis'] = (np.repeat(vc, 6, 0), np.tile(axes, (len(vc), 1)), 0.0)
    c = tri.reshape(-1, 3).mean(0)
    sets['inside'] = (c + rng.uniform(-0.05, 0.05, (300, 3)), unit(300), 0.0)
    far = rng.uniform(2.0, 3.0, (200, 3)) * rng.choice([-1.0, 1.0], (200, 3))
    sets['miss_root'] = (far, far / np.linalg.norm(far, axis=1, keepdims=True), 0.0)     # pointing away from the mesh
    sets['t_min'] = (rng.uniform(-0.5, 0.5, (500, 3)), unit(500), 0.3)
    for n in (0, 1, 63):
        sets[f'n{n}'] = (rng.uniform(-0.5, 0.5, (n, 3)), unit(n), 0.0)
    return {k: (np.ascontiguousarray(o, np.float32).reshape(-1, 3), np.ascontiguousarray(d, np.float32).reshape(-1, 3), t) for k, (o, d, t) in sets.items()}


MESHES = meshes()
