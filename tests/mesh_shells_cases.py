"""Case generators for tests/test_mesh_shells_*.py (include/rho2sdf_hip.h, r2s_mesh_shells).  Meshes are (verts (nv, 3) float32,
tris (nt, 3) int32, 0-based).  The extracted cases are iso-surfaces of the fields below on one lattice; their triangles are
recorded in tests/golden/mesh_shells_tris.npz (written by tests/golden/make_mesh_shells_cases.py from the library's own
extraction), their vertices are restated by iso_ref.vertices, so the tests without a GPU see the same meshes."""
import os

import numpy as np

import iso_ref as R
import mesh_query_cases as Q

ORIGIN, SPACING = (-1.0, 0.5, 0.25), 0.25
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mesh_shells_tris.npz")


def _mesh(V, T):
    return np.asarray(V, np.float32).reshape(-1, 3), np.asarray(T, np.int32).reshape(-1, 3)


def empty():
    return _mesh([], [])


def one_triangle():
    return _mesh([[0, 0, 0], [1, 0, 0], [0, 1, 0.5]], [[0, 1, 2]])


def all_collapsed():
    return _mesh([[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[0, 0, 1], [1, 2, 2], [0, 1, 0], [2, 2, 2]])


TET = [[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]]   # outward for the corner tetrahedron 0, e_x, e_y, e_z


def tetrahedron(L=60.0):
    """the corner tetrahedron of side L = 60: the reference point is (30, 30, 30), every A, B, C is +-30, so det, det * S and
    det * Q are integers divisible by 6, 24 and 120: every volume and moment term is exact"""
    return _mesh([[0, 0, 0], [L, 0, 0], [0, L, 0], [0, 0, L]], TET)


def cube(lo, side, reverse=False):
    x0, y0, z0 = lo
    V = [[x0 + side * i, y0 + side * j, z0 + side * k] for k in (0, 1) for j in (0, 1) for i in (0, 1)]
    T = np.array([[0, 2, 1], [1, 2, 3], [4, 5, 6], [5, 7, 6], [0, 1, 4], [1, 5, 4], [2, 6, 3], [3, 6, 7], [0, 4, 2], [2, 4, 6],
                  [1, 3, 5], [3, 7, 5]])
    return _mesh(V, T[:, ::-1] if reverse else T)


def join(*meshes):
    V, T, off = [], [], 0
    for v, t in meshes:
        V.append(v)
        T.append(t + off)
        off += len(v)
    return _mesh(np.concatenate(V), np.concatenate(T))


def cube_with_void():
    """a cube of side 2 holding a reversed cube of side 1"""
    return join(cube((0, 0, 0), 2.0), cube((0.5, 0.5, 0.5), 1.0, reverse=True))


def two_tets_sharing_vertex():
    V = [[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [-1, 0, 0], [0, -1, 0], [0, 0, -1]]
    T2 = [[0, 5, 4], [0, 4, 6], [0, 6, 5], [4, 5, 6]]
    return _mesh(V, TET + T2)


def three_on_edge():
    return _mesh([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, -1, 0.5], [0, 0, -1]], [[0, 1, 2], [0, 1, 3], [1, 0, 4]])


def triangle_twice():
    V, T = one_triangle()
    return V, np.concatenate([T, T])


def cube_one_reversed():
    V, T = cube((0, 0, 0), 1.5)
    T = T.copy()
    T[5] = T[5, ::-1]
    return V, T


def torus(n=8, m=8):
    """an n x m torus of quads, two triangles each"""
    u, v = np.meshgrid(2 * np.pi * np.arange(n) / n, 2 * np.pi * np.arange(m) / m, indexing="ij")
    V = np.stack([(2 + 0.7 * np.cos(v)) * np.cos(u), (2 + 0.7 * np.cos(v)) * np.sin(u), 0.7 * np.sin(v)], -1).reshape(-1, 3)
    T = []
    for i in range(n):
        for j in range(m):
            a, b, c, d = i * m + j, ((i + 1) % n) * m + j, ((i + 1) % n) * m + (j + 1) % m, i * m + (j + 1) % m
            T += [[a, b, c], [a, c, d]]
    return _mesh(V, T)


def ribbon(n=20000):
    """a strip of n triangles in index order: triangle t shares an edge with t - 1 and t + 1"""
    k = np.arange(n // 2 + 1)
    V = np.empty((2 * len(k), 3))
    V[0::2] = np.stack([0.01 * k, np.zeros(len(k)), 0.05 * np.sin(0.01 * k)], -1)
    V[1::2] = np.stack([0.01 * k, np.ones(len(k)), 0.05 * np.cos(0.01 * k)], -1)
    q = 2 * np.arange(n // 2)
    T = np.stack([np.stack([q, q + 1, q + 2], -1), np.stack([q + 1, q + 3, q + 2], -1)], 1).reshape(-1, 3)
    return _mesh(V, T)


def permuted(mesh, seed):
    """(mesh with its triangles under a seeded shuffle, perm): new triangle k is old triangle perm[k]"""
    V, T = mesh
    perm = np.random.default_rng(seed).permutation(len(T))
    return (V, np.ascontiguousarray(T[perm])), perm


def disjoint(n=3000, seed=11):
    rng = np.random.default_rng(seed)
    c = rng.uniform(-2.0, 2.0, (n, 1, 3))
    return Q.soup((c + 0.1 * rng.normal(size=(n, 3, 3))).tolist())


def fans(kmax=400):
    """triangle fans of 1, 2, .., kmax triangles laid end to end: shells whose segments straddle every block boundary"""
    V, T, off = [], [], 0
    for k in range(1, kmax + 1):
        a = np.pi * np.arange(k + 1) / k
        rim = np.stack([2.5 * k + np.cos(a), np.sin(a), 0.1 * np.sin(3 * a)], -1)
        V += [np.array([[2.5 * k, 0.0, 0.3]]), rim]
        i = np.arange(k)
        T.append(np.stack([np.full(k, off), off + 1 + i, off + 2 + i], -1))
        off += k + 2
    return _mesh(np.concatenate(V), np.concatenate(T))


def nested_field(n=41):
    """a ball (radius 17) holding a hollow (11) that holds a smaller ball (6), on an n^3 lattice of unit spacing"""
    g = np.arange(n, dtype=np.float64)
    c = (n - 1) / 2
    z, y, x = np.meshgrid(g, g, g, indexing="ij")
    d = np.sqrt((x - c) ** 2 + (y - c) ** 2 + (z - c) ** 2)
    return np.maximum(np.minimum(17.0 - d, d - 11.0), 6.0 - d).astype(np.float32).ravel()


def noise_field(n=24, seed=5, closed=True):
    """standard normal noise - 0.9: about 18 % of the points are interior, below the percolation threshold of the lattice, so
    the interior falls into many small bodies"""
    f = (np.random.default_rng(seed).normal(size=(n, n, n)) - 0.9).astype(np.float32)
    if closed:   # the border layer is exterior: every shell closes inside the lattice
        f[0], f[-1], f[:, 0], f[:, -1], f[:, :, 0], f[:, :, -1] = (np.float32(-1.0),) * 6
    return f.ravel()


def fields():
    """name -> (n, flattened field) of the extracted cases (iso 0, lattice (n, n, n), ORIGIN, SPACING)"""
    return {"sphere33": (33, Q.sphere_field(33, 12.3, np.float32)), "nested41": (41, nested_field()),
            "gyroid17": (17, R.gyroid(17, 12).ravel()), "noise24_closed": (24, noise_field()),
            "noise24_open": (24, noise_field(closed=False))}


_extracted = {}


def extracted(name):
    """the recorded mesh of an extracted case"""
    if name not in _extracted:
        n, f = fields()[name]
        V, _ = R.vertices(f, (n, n, n), ORIGIN, SPACING, 0.0)
        with np.load(GOLDEN) as g:
            _extracted[name] = (V, g[name].astype(np.int32))
    return _extracted[name]


HAND = {"empty": empty, "one_triangle": one_triangle, "all_collapsed": all_collapsed, "tetrahedron": tetrahedron,
        "cube_with_void": cube_with_void, "two_tets_sharing_vertex": two_tets_sharing_vertex, "three_on_edge": three_on_edge,
        "triangle_twice": triangle_twice, "cube_one_reversed": cube_one_reversed, "torus": torus, "ribbon": ribbon,
        "ribbon_reversed": lambda: (ribbon()[0], np.ascontiguousarray(ribbon()[1][::-1])),
        "ribbon_shuffled": lambda: permuted(ribbon(), 21)[0], "disjoint": disjoint, "fans": fans}
EXTRACTED = ("sphere33", "nested41", "gyroid17", "noise24_closed", "noise24_open")
ALL = tuple(HAND) + EXTRACTED

_cases = {}


def case(name):
    if name not in _cases:
        _cases[name] = HAND[name]() if name in HAND else extracted(name)
    return _cases[name]
