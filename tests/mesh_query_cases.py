"""Case generators for tests/test_mesh_query_*.py: meshes that stress the tree of the mesh index (include/rho2sdf_hip.h,
r2s_mesh_index) and the point sets they are queried with.  Meshes are (verts (nv, 3) float32, tris (nt, 3) int32, 0-based)."""
import numpy as np


def sphere_field(n, r, dtype):
    """r - |x - c| on an n^3 lattice of unit spacing, c the lattice centre, flattened x fastest"""
    g = np.arange(n, dtype=np.float64)
    c = (n - 1) / 2
    z, y, x = np.meshgrid(g, g, g, indexing="ij")
    return (r - np.sqrt((x - c) ** 2 + (y - c) ** 2 + (z - c) ** 2)).astype(dtype).ravel()


def soup(tri_list):
    """unwelded triangles [(a, b, c), ...] -> (verts, tris)"""
    V = np.array([p for t in tri_list for p in t], np.float32).reshape(-1, 3)
    return V, np.arange(len(V), dtype=np.int32).reshape(-1, 3)


def first_triangles(n, seed=1):
    """n = 0, 1, 2, 3 random triangles in [0, 1]^3 over a shared pool of vertices"""
    rng = np.random.default_rng(seed)
    V = rng.uniform(0.0, 1.0, size=(7, 3)).astype(np.float32)
    T = np.array([[0, 1, 2], [2, 3, 4], [4, 5, 6]], np.int32)[:n]
    return V, T


def box_points(lo, hi, n, seed):
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    return np.random.default_rng(seed).uniform(lo, hi, size=(n, 3))


def far_points(lo, hi, n, seed, factor=1e3):
    """points at `factor` times the box size from its centre, in random directions"""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    u = np.random.default_rng(seed).normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    return 0.5 * (lo + hi) + factor * float((hi - lo).max()) * u


def bad_rows():
    """rows with a non-finite coordinate: the answer is NaN / -1"""
    return np.array([[np.nan, 0.0, 0.0], [0.0, np.inf, 0.0], [0.0, 0.0, -np.inf], [np.nan, np.nan, np.nan], [np.inf, 1.0, np.nan]])


def planar(n=24, seed=4):
    """every triangle in the plane z = 0.5: one axis of the mesh box has zero extent"""
    rng = np.random.default_rng(seed)
    tl = []
    for _ in range(n):
        c = rng.uniform(0.0, 2.0, 2)
        p = c + rng.normal(size=(3, 2)) * 0.2
        tl.append([(p[k, 0], p[k, 1], 0.5) for k in range(3)])
    return soup(tl)


def degenerate(seed=6):
    """ordinary triangles mixed with zero-area ones (collinear, two equal, all equal vertices), coincident vertices and
    triangles given twice"""
    rng = np.random.default_rng(seed)
    tl = []
    for _ in range(30):
        a = np.float32(rng.uniform(-1.0, 2.0, 3)).astype(np.float64)
        e = np.array([0.25, -0.5, 0.125])
        tl += [(a, a + e, a + 2 * e), (a, a, a + e), (a, a, a)]
        c = rng.uniform(-1.0, 2.0, 3)
        tl.append(tuple(c + rng.normal(size=3) * 0.3 for _ in range(3)))
    V, T = soup(tl)
    return V, np.concatenate([T, T[::7]])


def cascade(seed=8):
    """triangles of size 2^-k with centres at x = 2^-k, k = 0..20, plus 2000 tiny triangles inside one Morton cell: a deep,
    one-sided tree"""
    rng = np.random.default_rng(seed)
    tl = []
    for k in range(21):
        s = 2.0 ** -k
        c = np.array([s, 0.3 * s, 0.2 * s])
        tl.append(tuple(c + 0.25 * s * rng.normal(size=3) for _ in range(3)))
    for _ in range(2000):
        c = np.array([0.7, 0.7, 0.7]) + rng.uniform(0.0, 1e-4, 3)
        tl.append(tuple(c + 2e-5 * rng.normal(size=3) for _ in range(3)))
    return soup(tl)


def scale_mix(seed=9):
    """two triangles spanning the whole unit box over a cluster of 5000 triangles of 1e-3 the box size: boxes overlap everywhere"""
    rng = np.random.default_rng(seed)
    tl = [((0, 0, 0), (1, 1, 0), (1, 0, 1)), ((0, 1, 1), (1, 0, 0), (0, 0, 1))]
    for _ in range(5000):
        c = rng.uniform(0.3, 0.7, 3)
        tl.append(tuple(c + 1e-3 * rng.normal(size=3) for _ in range(3)))
    return soup(tl)
