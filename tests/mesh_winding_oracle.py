"""TEST INFRASTRUCTURE ONLY -- fp64 numpy reference of the generalized winding number (csrc/dsdf_winding.h: tri_solid_angle, bvh_winding),
and the shared inputs of its CPU and GPU tests.  Nothing under differentiable-sdf-rendering_amd/ imports it.

The formulation differs from the kernel's on purpose (a shared mistake must not hide): the kernel takes the solid angle of a triangle from
Van Oosterom & Strackee's one atan2 of a triple product over a sum of lengths and dot products; here it is the SPHERICAL EXCESS of the
triangle's projection onto the unit sphere around the point, A + B + C - pi, with the three dihedral angles between the planes through the
point and two corners each (angle between the plane normals, from atan2(|n1 x n2|, n1 . n2)), signed by the side of the point."""
import functools

import numpy as np

import mesh_closest_oracle as C
import mesh_oracle as M

# max |w_fp32 - w_fp64| of the HOST build of csrc/dsdf_winding.h's exact sum over every mesh and point set below
# (`PYTHONPATH=oracle:tests python tests/test_mesh_winding_host.py` prints it), and the gate of every comparison of an exact sum with this
# reference: 4 x the measurement -- the factor covers other random draws and the device's atan2f, not other arithmetic.
MEASURED_MAX_ERR = 2.861e-06
GATE = 4 * MEASURED_MAX_ERR
TREE_GATE = 0.1          # the CONDITION on the dipole approximation at the default beta = 2 against the exact sum: 0.4 left to the threshold 0.5
BETAS = (2.0, 3.0, 4.0)


def _angle(u, v):
    return np.arctan2(np.linalg.norm(np.cross(u, v), axis=-1), (u * v).sum(-1))


def solid_angle(points, tri):
    """Signed solid angle of the triangles tri (..., 3, 3) seen from points (..., 3) (broadcast against each other), in fp64: positive on
    the side the normal (p1 - p0) x (p2 - p0) points away from.  0 where the point lies in the plane of the triangle."""
    x, tri = np.asarray(points, np.float64), np.asarray(tri, np.float64)
    a, b, c = tri[..., 0, :] - x, tri[..., 1, :] - x, tri[..., 2, :] - x
    nab, nbc, nca = np.cross(a, b), np.cross(b, c), np.cross(c, a)
    # the dihedral angle along a is the angle between the planes (a, b) and (a, c): between a x b and a x c = -(c x a)
    excess = _angle(nab, -nca) + _angle(nbc, -nab) + _angle(nca, -nbc) - np.pi
    det = (a * nbc).sum(-1)
    flat = (np.linalg.norm(nab, axis=-1) == 0) | (np.linalg.norm(nbc, axis=-1) == 0) | (np.linalg.norm(nca, axis=-1) == 0) | (det == 0)
    return np.where(flat, 0.0, np.sign(det) * excess)


def winding(points, tri, block=256):
    """(n,) fp64: the sum of solid_angle over all triangles, over 4 pi."""
    x = np.asarray(points, np.float64).reshape(-1, 3)
    tri = np.asarray(tri, np.float64).reshape(-1, 3, 3)
    w = np.empty(len(x))
    for s in range(0, len(x), block):
        w[s:s + block] = solid_angle(x[s:s + block, None, :], tri[None]).sum(1)
    return w / (4 * np.pi)


# ---- shared inputs ------------------------------------------------------------------------------------------------------------------
def _ico(radius, subdiv, centre=(0.0, 0.0, 0.0)):
    v, f = M.icosphere(radius, subdiv, centre=centre)
    return np.ascontiguousarray(v[f], np.float32)


# the two spheres of the soup and what they say about a point: the number of spheres it is inside of
TWO = (((-0.1, 0.0, 0.0), 0.3), ((0.15, 0.05, 0.0), 0.25))


def meshes():
    out = dict(C.MESHES)                                  # T1, T4, T5, box12, ico20 / 80 / 320, degenerate: open and closed
    out['two_spheres'] = np.concatenate([_ico(r, 2, c) for c, r in TWO])            # one soup, overlapping: w in {0, 1, 2}
    ico = C.MESHES['ico320']
    out['half_ico'] = np.ascontiguousarray(ico[ico.mean(1) @ CAP_AXIS > 0])        # open: the faces on one side of a plane through the centre
    out['ico320_hole'] = np.ascontiguousarray(np.delete(ico, HOLE, 0))              # one triangle removed
    return {k: np.ascontiguousarray(v, np.float32) for k, v in out.items()}


HOLE = 17
CAP_AXIS = np.asarray([0.2, 0.3, 1.0])      # (no face of the icosphere has its centroid IN this plane: 160 faces on either side)
MESHES = meshes()
CLOSED = ('box12', 'ico20', 'ico80', 'ico320', 'two_spheres')


def query_points(tri, seed, n_random=20000):
    """mesh_closest_oracle.query_points WITHOUT the sets on the surface, plus points +-1e-3 along the normal from (up to) 200 centroids."""
    sets = {k: v for k, v in C.query_points(tri, seed, n_random).items() if k not in ON_SURFACE}
    t = np.asarray(tri, np.float64)
    n = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    ln = np.linalg.norm(n, axis=1)
    ok = np.nonzero(ln > 0)[0][:200]
    g, n = t[ok].mean(1), n[ok] / ln[ok, None]
    sets['near'] = np.concatenate([g + 1e-3 * n, g - 1e-3 * n]).astype(np.float32)
    return sets


ON_SURFACE = ('vertices', 'midpoints', 'centroids')


def all_points(tri, seed, n_random=20000):
    return np.concatenate(list(query_points(tri, seed, n_random).values()))


@functools.lru_cache(maxsize=None)
def points_and_reference(name):
    """(points, fp64 winding numbers) of a shared mesh, computed once per process: 20000 uniform points for the meshes of up to 100
    triangles, 5000 for the larger ones (the reference is every point against every triangle), plus the other sets."""
    tri = MESHES[name]
    pts = all_points(tri, len(name), 20000 if tri.shape[0] <= 100 else 5000)
    return pts, winding(pts, tri)


def surface_points(tri, seed):
    return np.concatenate([C.query_points(tri, seed, 1)[k] for k in ON_SURFACE])


def _parts(name):
    return (MESHES[name][:320], MESHES[name][320:]) if name == 'two_spheres' else (MESHES[name],)


def analytic_count(name, pts):
    """The integer winding number of box12 / ico320 / two_spheres without any solid angle: every part is a CONVEX polyhedron with outward
    normals, and a point is inside one exactly when it is behind the plane of every face; the count is the number of parts it is inside
    of.  -> (count, sure): sure marks the points farther than 1e-3 from the surface (mesh_closest_oracle.closest, fp64)."""
    x = np.asarray(pts, np.float64)
    count = np.zeros(len(x), int)
    for part in _parts(name):
        t = part.astype(np.float64)
        n = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
        h = ((x[:, None, :] - t[None, :, 0, :]) * n[None]).sum(-1)
        count += (h < 0).all(1)
    return count, C.closest(x, MESHES[name])[0] > 1e-3
