"""Named cases of the winding tests (tests/test_mesh_winding_cpu.py, tests/test_mesh_winding_gpu.py): tiny meshes with an analytic
inside, the point sets that go with them, and the sphere iso-surfaces whose field gives the sign at every lattice point.

case(name) -> (V float32 (nv, 3), T int32 (nt, 3)); points(name) -> float64 (n, 3); lattice(name) -> (dims, origin, spacing) or
None; truth(name, P) -> the analytic winding at P, or None; on_surface(name, P) -> bool mask of the points the truth leaves out.
expected(name, ray) -> the restatement's (winding, crossings) at points(name), computed once."""
import functools

import numpy as np

import mesh_winding_ref as R

FACE_QUAD = ((0, 1, 2), (0, 2, 3))


def box_mesh(lo, hi, n, outward=True):
    """the surface of the box [lo, hi]^3 with n x n quads per face, each split in two; wound outward (or inward)"""
    lo, hi = np.broadcast_to(np.asarray(lo, float), 3), np.broadcast_to(np.asarray(hi, float), 3)
    V, T, ids = [], [], {}

    def vid(p):
        key = tuple(np.round(p, 9))
        if key not in ids:
            ids[key] = len(V)
            V.append(p)
        return ids[key]
    for axis in range(3):
        u, v = (axis + 1) % 3, (axis + 2) % 3
        for sgn in (0, 1):
            for i in range(n):
                for j in range(n):
                    q = []
                    for di, dj in ((0, 0), (1, 0), (1, 1), (0, 1)):
                        p = np.empty(3)
                        p[axis] = hi[axis] if sgn else lo[axis]
                        p[u] = lo[u] + (hi[u] - lo[u]) * (i + di) / n
                        p[v] = lo[v] + (hi[v] - lo[v]) * (j + dj) / n
                        q.append(vid(p))
                    if not sgn:                       # the quad above has the normal +e_axis
                        q = q[::-1]
                    T += [[q[a], q[b], q[c]] for a, b, c in FACE_QUAD]
    V, T = np.array(V, np.float32), np.array(T, np.int32)
    return V, (T if outward else T[:, ::-1].copy())


def octahedron(r, outward=True):
    """|p|_1 = r"""
    V = np.array([[r, 0, 0], [-r, 0, 0], [0, r, 0], [0, -r, 0], [0, 0, r], [0, 0, -r]], np.float32)
    T = []
    for sx in (0, 1):
        for sy in (2, 3):
            for sz in (4, 5):
                tri = [sx, sy, sz]
                n = np.cross(V[sy] - V[sx], V[sz] - V[sx])
                if np.dot(n, V[sx] + V[sy] + V[sz]) < 0:
                    tri = tri[::-1]
                T.append(tri)
    T = np.array(T, np.int32)
    return V, (T if outward else T[:, ::-1].copy())


def merged(*meshes):
    V, T, off = [], [], 0
    for v, t in meshes:
        V.append(v)
        T.append(t + off)
        off += len(v)
    return np.concatenate(V).astype(np.float32), np.concatenate(T).astype(np.int32)


def in_box(P, lo, hi):
    return ((P > lo) & (P < hi)).all(axis=1).astype(np.int32)


def on_box(P, lo, hi):
    return ((P >= lo) & (P <= hi)).all(axis=1) & ((P == lo) | (P == hi)).any(axis=1)


ANALYTIC = ["empty", "one_triangle", "tetrahedron", "cube22", "octahedra", "two_cubes", "inward_cube", "reversed_cube", "collapsed_cube"]
SPHERES = ["sphere17", "sphere33", "sphere_far"]
ALL = ANALYTIC + SPHERES
CLOSED = ["tetrahedron", "cube22", "octahedra", "two_cubes", "inward_cube", "collapsed_cube"]   # consistent windings: all six rays agree


@functools.lru_cache(maxsize=None)
def case(name):
    if name == "empty":
        return np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)
    if name == "one_triangle":
        return np.array([[0, 0, 0], [2, 0, 0.5], [0, 2, 1]], np.float32), np.array([[0, 1, 2]], np.int32)
    if name == "tetrahedron":
        return np.array([[0, 0, 0], [2, 0, 0], [0, 2, 0], [0, 0, 2]], np.float32), np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], np.int32)
    if name == "cube22":
        return box_mesh(0, 2, 2)
    if name == "octahedra":
        return merged(octahedron(2.0), octahedron(0.5, outward=False))
    if name == "two_cubes":
        return merged(box_mesh(0, 2, 2), box_mesh(1, 3, 2))
    if name == "inward_cube":
        return box_mesh(0, 2, 2, outward=False)
    if name == "reversed_cube":
        V, T = box_mesh(0, 2, 2)
        flip = np.random.default_rng(30).random(len(T)) < 0.3
        T = T.copy()
        T[flip] = T[flip][:, ::-1]
        return V, T
    if name == "collapsed_cube":
        V, T = box_mesh(0, 2, 2)
        return V, np.concatenate([T, np.array([[0, 5, 5]], np.int32)])
    raise KeyError(name)          # (the spheres come from the GPU: sphere_case)


def lattice(name):
    if name in ("cube22", "inward_cube", "reversed_cube", "collapsed_cube"):
        return (7, 7, 7), (-0.5, -0.5, -0.5), 0.5            # the half-integer lattice -0.5 .. 2.5
    if name == "two_cubes":
        return (9, 9, 9), (-0.5, -0.5, -0.5), 0.5
    if name == "octahedra":
        return (21, 21, 21), (-2.5, -2.5, -2.5), 0.25        # the quarter-integer lattice -2.5 .. 2.5
    if name in ("one_triangle", "tetrahedron"):
        return (2, 65, 5), (-0.25, -0.25, -0.25), 0.04       # rows of 2 along x, of 65 along y
    if name == "empty":
        return (2, 3, 2), (0.0, 0.0, 0.0), 1.0
    return None


def lattice_points(lat):
    dims, origin, h = lat
    k, j, i = np.meshgrid(np.arange(dims[2]), np.arange(dims[1]), np.arange(dims[0]), indexing="ij")
    return np.stack([origin[0] + h * i.ravel().astype(float), origin[1] + h * j.ravel().astype(float), origin[2] + h * k.ravel().astype(float)],
                    axis=1)


@functools.lru_cache(maxsize=None)
def points(name):
    """the case's lattice, then 65 seeded random points around the mesh, then NaN / inf rows"""
    V, _ = case(name)
    lo, hi = (V.min(axis=0), V.max(axis=0)) if len(V) else (np.zeros(3), np.ones(3))
    rng = np.random.default_rng(len(name) + 7)
    rnd = rng.uniform(lo - 0.3, hi + 0.3, size=(65, 3))
    bad = np.array([[np.nan, 0.5, 0.5], [0.5, np.inf, 0.5], [0.5, 0.5, -np.inf]])
    return np.concatenate([lattice_points(lattice(name)), rnd, bad])


def truth(name, P):
    """the analytic winding at P (None: the case has none); valid off the surface only"""
    l1 = np.abs(P).sum(axis=1)
    if name in ("cube22", "collapsed_cube"):
        return in_box(P, 0, 2)
    if name == "inward_cube":
        return -in_box(P, 0, 2)
    if name == "two_cubes":
        return in_box(P, 0, 2) + in_box(P, 1, 3)
    if name == "octahedra":
        return (l1 < 2).astype(np.int32) - (l1 < 0.5).astype(np.int32)
    if name == "tetrahedron":
        return ((P > 0).all(axis=1) & (P.sum(axis=1) < 2)).astype(np.int32)
    if name == "empty":
        return np.zeros(len(P), np.int32)
    return None


def on_surface(name, P):
    l1 = np.abs(P).sum(axis=1)
    bad = ~np.isfinite(P).all(axis=1)
    if name in ("cube22", "collapsed_cube", "inward_cube", "reversed_cube"):
        return bad | on_box(P, 0, 2)
    if name == "two_cubes":
        return bad | on_box(P, 0, 2) | on_box(P, 1, 3)
    if name == "octahedra":
        return bad | (l1 == 2) | (l1 == 0.5)
    if name == "tetrahedron":
        inside_closed = (P >= 0).all(axis=1) & (P.sum(axis=1) <= 2)
        return bad | (inside_closed & ((P == 0).any(axis=1) | (P.sum(axis=1) == 2)))
    return bad


@functools.lru_cache(maxsize=None)
def expected(name, ray):
    V, T = case(name)
    return R.winding_ref(V, T, points(name), ray)


# ---- the sphere iso-surfaces (the mesh comes from r2s_extract_isosurface: these need the GPU) -----------------------------

SPHERE_SPEC = {   # cells per side, spacing, the lattice's corner; the centre is the middle lattice point
    "sphere17": (16, 0.125, (0.0, 0.0, 0.0)),
    "sphere33": (32, 0.0625, (-1.0, -1.0, -1.0)),
    "sphere_far": (32, 0.1, (1e3 - 1.6, -2e3 - 1.6, 5e2 - 1.6)),
}


def sphere_field(name):
    """-> (dims, origin, h, f (nz, ny, nx) float64): f = r - |p - c| on the lattice points as the library forms them.  The
    squared distances of lattice points from a lattice point are h^2 times integers, so r = h sqrt(m + 1/2) keeps every lattice
    point away from the level: asserted below, min |f| >= 1e-3 h."""
    n, h, origin = SPHERE_SPEC[name]
    dims = (n + 1,) * 3
    P = lattice_points((dims, origin, h))
    c = P[((n // 2) * dims[1] + n // 2) * dims[0] + n // 2]
    cells = 0.375 * n                                        # the radius in cells: 6 of 16, 12 of 32: strictly inside the lattice
    r = h * np.sqrt(np.floor(cells * cells) + 0.5)
    f = r - np.sqrt(((P - c) ** 2).sum(axis=1))
    assert np.abs(f).min() >= 1e-3 * h, (name, np.abs(f).min(), h)
    return dims, origin, h, f.reshape(dims[2], dims[1], dims[0])


def raw_grid(pkg, dims, origin, h):
    """the Grid whose lattice is exactly (dims, origin, h)"""
    g = pkg._lib.R2SGrid()
    for a in range(3):
        g.aabb_min[a], g.N[a], g.aabb_max[a] = origin[a], dims[a] - 1, origin[a] + h * (dims[a] - 1)
    g.cell_size, g.ngp = h, dims[0] * dims[1] * dims[2]
    return pkg.Grid(None, None, 0, _raw=g)


_spheres = {}


def sphere_case(pkg, name):
    """-> dict(V, T, grid, lattice, f): the surface r2s_extract_isosurface returns for the sphere field, once per session"""
    if name not in _spheres:
        dims, origin, h, f = sphere_field(name)
        grid = raw_grid(pkg, dims, origin, h)
        V, T = pkg.extract_isosurface(f, grid, iso=0.0, device=0)
        _spheres[name] = dict(V=V, T=T, grid=grid, lattice=(dims, origin, h), f=f)
    return _spheres[name]
