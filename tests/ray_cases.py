"""Ray sets for tests/test_ray_*.py (include/rho2sdf_hip.h, r2s_mesh_index_raycast): every function returns
(origins (n, 3) float64, directions (n, 3) float64) for a mesh (verts float32, tris int32); the meshes are those of
tests/mesh_query_cases.py plus the closed sphere surface below."""
import numpy as np

import iso_ref
import mesh_query_cases as C


def mesh_box(V):
    V = np.asarray(V, np.float64).reshape(-1, 3)
    if len(V) == 0:
        return np.zeros(3), np.ones(3)
    return V.min(axis=0), V.max(axis=0)


def uniform(V, n, seed):
    """uniform origins in 1.5x the mesh box, normally distributed directions"""
    lo, hi = mesh_box(V)
    c, e = 0.5 * (lo + hi), np.maximum(hi - lo, 1e-3 * max(float(np.abs(hi - lo).max()), 1.0))
    rng = np.random.default_rng(seed)
    return c + 0.75 * e * rng.uniform(-1.0, 1.0, size=(n, 3)), rng.normal(size=(n, 3))


def aligned(V, n, seed):
    """axis-aligned and plane-aligned directions: two or one exact zero components"""
    o, d = uniform(V, n, seed)
    rng = np.random.default_rng(seed + 1000)
    for i in range(n):
        if i % 2 == 0:
            keep = rng.integers(3)
            d[i, [k for k in range(3) if k != keep]] = 0.0
        else:
            d[i, rng.integers(3)] = 0.0
    return o, d


def aimed(origins, targets):
    """rays from origins (cycled) at the float64 targets, d = target - origin"""
    targets = np.asarray(targets, np.float64).reshape(-1, 3)
    o = np.asarray(origins, np.float64).reshape(-1, 3)
    o = o[np.arange(len(targets)) % len(o)]
    return o, targets - o


def edge_midpoints(V, T):
    v = np.asarray(V, np.float32).astype(np.float64)
    T = np.asarray(T, np.int64)
    e = np.sort(np.concatenate([T[:, [0, 1]], T[:, [1, 2]], T[:, [2, 0]]]), axis=1)
    e = np.unique(e, axis=0)
    return 0.5 * (v[e[:, 0]] + v[e[:, 1]])


def centroids(V, T):
    v = np.asarray(V, np.float32).astype(np.float64)
    T = np.asarray(T, np.int64)
    return (v[T[:, 0]] + v[T[:, 1]] + v[T[:, 2]]) / 3.0


def inner_origins(centre, radius, n, seed):
    """origins within a quarter of the radius of the centre"""
    rng = np.random.default_rng(seed)
    u = rng.normal(size=(n, 3))
    u *= (0.25 * radius * rng.uniform(0.0, 1.0, n) ** (1 / 3) / np.linalg.norm(u, axis=1))[:, None]
    return np.asarray(centre, np.float64) + u


def from_vertices(V, n, seed):
    """rays that start exactly on vertices"""
    v = np.asarray(V, np.float32).astype(np.float64)
    rng = np.random.default_rng(seed)
    pick = rng.integers(len(v), size=n)
    return v[pick], rng.normal(size=(n, 3))


def far(V, n, seed, factor=1e3):
    """origins at `factor` box sizes, aimed at uniform points of the box"""
    lo, hi = mesh_box(V)
    o = C.far_points(lo, hi, n, seed, factor)
    tgt = C.box_points(lo, hi, n, seed + 1)
    return o, tgt - o


def bad():
    """NaN, inf and zero directions, non-finite origins: NaN / -1 / 0"""
    o = np.array([[0.1, 0.2, 0.3]] * 6)
    d = np.array([[np.nan, 0.0, 1.0], [np.inf, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, -0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    o[4, 1] = np.nan
    o[5, 2] = -np.inf
    return o, d


def families(V, T, n, seed, closed_centre=None):
    """all families on one mesh, n rays per random family (targets thinned to at most n)"""
    parts = [uniform(V, n, seed), aligned(V, n, seed + 1), far(V, max(n // 4, 8), seed + 3), bad()]
    if len(V):
        parts.append(from_vertices(V, n, seed + 2))
    if len(T):
        lo, hi = mesh_box(V)
        org = C.box_points(lo - 0.25 * (hi - lo) - 0.1, hi + 0.25 * (hi - lo) + 0.1, 16, seed + 4) if closed_centre is None \
            else inner_origins(closed_centre[0], closed_centre[1], 16, seed + 4)
        for tg in (np.asarray(V, np.float32).astype(np.float64), edge_midpoints(V, T), centroids(V, T)):
            tg = tg[:: max(1, len(tg) // n)]
            parts.append(aimed(org, tg))
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def sphere_vertices(n, r=None, origin=(-3.0, 1.5, 0.25), h=0.25):
    """the iso-surface vertices (tests/iso_ref.py) of a sphere field on an n^3 lattice -> (verts float32, centre, radius)"""
    r = 0.325 * (n - 1) if r is None else r
    f = C.sphere_field(n, r, np.float32)
    V, _ = iso_ref.vertices(f, (n, n, n), origin, h, 0.0)
    return V, np.asarray(origin) + h * (n - 1) / 2, h * r


def closed_sphere(n):
    """a closed, outward-wound triangle surface over the iso_ref vertices of the n^3 sphere field: the surface is star-shaped
    about the lattice centre, so the convex hull of the vertices' directions from the centre triangulates it without gaps
    -> (verts float32, tris int32, centre, radius)"""
    from scipy.spatial import ConvexHull
    V, c, rad = sphere_vertices(n)
    u = V.astype(np.float64) - c
    u /= np.linalg.norm(u, axis=1)[:, None]
    T = ConvexHull(u).simplices.astype(np.int64)
    v = V.astype(np.float64)
    nrm = np.cross(v[T[:, 1]] - v[T[:, 0]], v[T[:, 2]] - v[T[:, 0]])
    flip = (nrm * (v[T].mean(axis=1) - c)).sum(axis=1) < 0.0
    T[flip] = T[flip][:, [0, 2, 1]]
    return V, T.astype(np.int32), c, rad
