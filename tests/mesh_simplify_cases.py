"""Named inputs of the mesh-simplify tests, each at the smallest size where its path can go wrong.  CASES: name -> (verts float32
(nv, 3), tris int32 (nt, 3), cell); permuted(case) gives the same mesh with its vertices and triangles shuffled and its corners
rotated.  PERMUTED names the half of the cases that also run that way (all_cases() yields both)."""
import numpy as np

F = np.float32


def _mesh(v, t):
    return np.ascontiguousarray(v, F).reshape(-1, 3), np.ascontiguousarray(t, np.int32).reshape(-1, 3)


def grid_patch(nx, ny, origin, du, dv):
    """(nx + 1) x (ny + 1) vertices origin + i du + j dv, two triangles a quad"""
    i, j = np.meshgrid(np.arange(nx + 1), np.arange(ny + 1), indexing="ij")
    v = np.asarray(origin, np.float64) + i[..., None] * np.asarray(du, np.float64) + j[..., None] * np.asarray(dv, np.float64)
    idx = lambda a, b: a * (ny + 1) + b
    t = []
    for a in range(nx):
        for b in range(ny):
            t += [[idx(a, b), idx(a + 1, b), idx(a + 1, b + 1)], [idx(a, b), idx(a + 1, b + 1), idx(a, b + 1)]]
    return v.reshape(-1, 3), np.array(t)


def cube(n=4, offset=(0.0, 0.0, 0.0)):
    """the unit cube, every edge divided n times: coordinates float32(k / n + offset) per axis, so that every face is exactly
    planar in float32; 12 n^2 triangles, outward, on shared vertices"""
    ax = [(np.arange(n + 1) / n + o).astype(F) for o in offset]
    ids, verts, tris = {}, [], []

    def vid(k):
        if k not in ids:
            ids[k] = len(verts)
            verts.append([ax[0][k[0]], ax[1][k[1]], ax[2][k[2]]])
        return ids[k]

    for axis in range(3):
        u, w = (axis + 1) % 3, (axis + 2) % 3
        for side in (0, n):
            for a in range(n):
                for b in range(n):
                    def corner(da, db):
                        k = [0, 0, 0]
                        k[axis], k[u], k[w] = side, a + da, b + db
                        return vid(tuple(k))
                    quad = [corner(0, 0), corner(1, 0), corner(1, 1), corner(0, 1)]
                    if side == 0:
                        quad = quad[::-1]
                    tris += [[quad[0], quad[1], quad[2]], [quad[0], quad[2], quad[3]]]
    return _mesh(verts, tris) + (ax,)


def icosphere(level=3):
    g = (1 + 5 ** 0.5) / 2
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1), (-g, 0, -1),
         (-g, 0, 1)]
    v = [np.array(p) / np.linalg.norm(p) for p in v]
    t = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4),
         (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(level):
        mid, nt = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[k] = len(v) - 1
            return mid[k]
        for a, b, c in t:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nt += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        t = nt
    return _mesh(v, t)


def fan(n, seed, ring=16):
    """a class of exactly n members: n vertices on a wobbling circle of radius 0.1 about (0.5, 0.5, 0.5), inside the cell [0, 1)^3,
    joined to a zig-zag ring of 16 vertices at radius 2.3, each in a cell of its own; the triangles with two inner corners
    collapse and still count once for the class"""
    rng = np.random.default_rng(seed)
    a = 2 * np.pi * np.arange(n) / n
    b = 2 * np.pi * (np.arange(ring) + 0.5) / ring
    inner = np.stack([0.5 + 0.1 * np.cos(a), 0.5 + 0.1 * np.sin(a), 0.5 + 0.05 * rng.uniform(-1, 1, n)], 1)
    outer = np.stack([0.5 + 2.3 * np.cos(b), 0.5 + 2.3 * np.sin(b), 0.5 + 0.4 * np.where(np.arange(ring) % 2, 1.0, -1.0)], 1)
    r = n + (np.arange(n) * ring) // n           # the ring vertex opposite inner vertex i
    t = []
    for i in range(n):
        j = (i + 1) % n
        t.append([i, r[i], j])
        if r[i] != r[j]:
            t.append([j, r[i], r[j]])
    return _mesh(np.concatenate([inner, outer]), t)


def permuted(case, seed=7):
    v, t, cell = case
    rng = np.random.default_rng(seed)
    pv = rng.permutation(len(v))                 # new vertex j is old vertex pv[j]
    inv = np.empty(len(v), np.int64)
    inv[pv] = np.arange(len(v))
    t2 = inv[t].reshape(-1, 3)[rng.permutation(len(t))] if len(t) else t
    t2 = np.array([np.roll(row, int(r)) for row, r in zip(t2, rng.integers(0, 3, len(t2)))], np.int32).reshape(-1, 3)
    return v[pv], t2, cell


def _cases():
    C = {}
    C["empty"] = _mesh([], []) + (1.0,)
    C["one_triangle_one_cell"] = _mesh([[0.1, 0.1, 0.1], [0.6, 0.2, 0.1], [0.2, 0.7, 0.3]], [[0, 1, 2]]) + (1.0,)
    C["one_triangle_three_cells"] = _mesh([[0.1, 0.1, 0.1], [1.6, 0.2, 0.1], [0.2, 1.7, 0.3]], [[0, 1, 2]]) + (1.0,)
    quad = [[0.2, 0.2, 0.2], [1.3, 0.4, 0.1], [0.5, 1.5, 0.3], [0.7, 1.2, 0.6]]          # (2 and 3 share a cell)
    C["duplicate_pair"] = _mesh(quad, [[0, 1, 2], [0, 1, 3]]) + (1.0,)
    C["opposite_pair"] = _mesh(quad, [[0, 1, 2], [1, 0, 3]]) + (1.0,)
    # cube: coordinates -0.2, 0.05, 0.3, 0.55, 0.8 per axis and cell 0.5: per axis the cells -1 | 0 0 | 1 1, so the corners at
    # 0.8 share their cell with edge and face vertices, the corners at -0.2 sit alone, and no face lies on a cell boundary
    v, t, _ = cube(4, (-0.2, -0.2, -0.2))
    C["cube"] = (v, t, 0.5)
    v, t, _ = cube(4, (1000.0, 1000.0, 1000.0))
    C["cube_far"] = (v, t, 0.1)
    v, t = grid_patch(8, 8, (0.03, 0.02, 0.3), (0.11, 0.01, 0.0), (-0.02, 0.12, 0.0))
    C["plane_patch"] = _mesh(v, t) + (0.3,)
    v1, t1 = grid_patch(8, 4, (0.03, 0.02, 0.1), (0.11, 0.0, 0.0), (0.0, 0.12, 0.0))      # z = 0.1, y in [0.02, 0.5]
    v2, t2 = grid_patch(8, 4, (0.03, 0.5, 0.1), (0.11, 0.0, 0.0), (0.0, 0.0, 0.13))       # y = 0.5, z in [0.1, 0.62]
    C["crease"] = _mesh(np.concatenate([v1, v2]), np.concatenate([t1, t2 + len(v1)])) + (0.3,)
    v, t = icosphere(3)
    v = (v.astype(np.float64) + (0.013, 0.027, 0.041)).astype(F)   # (off the lattice: no vertex on a cell face by symmetry)
    for cell in (0.5, 0.25, 0.1):
        C[f"icosphere_{cell}"] = (v, t, cell)
    b = [[0.0, 0.0, 0.0], [-0.0, 0.5, 1.0], [1.0, -0.0, 0.5], [0.5, 1.0, -0.0], [-0.0, -0.0, -0.0], [2.0, 1.0, 1.0], [-1.0, 0.5, -0.5],
         [0.5, -1.0, 2.0]]
    C["cell_boundaries"] = _mesh(b, [[0, 5, 6], [1, 2, 3], [4, 7, 5], [1, 6, 7], [2, 5, 7], [3, 6, 5]]) + (1.0,)
    # vertex 3 is referenced only by an input-collapsed triangle, vertex 4 by nothing
    C["non_members"] = _mesh([[0.1, 0.1, 0.1], [1.6, 0.2, 0.1], [0.2, 1.7, 0.3], [0.3, 0.3, 0.3], [1.5, 1.5, 1.5]],
                             [[0, 1, 2], [3, 3, 0]]) + (1.0,)
    for n in (255, 256, 257, 5000):
        C[f"fan_{n}"] = fan(n, n) + (1.0,)
    C["two_corners_one_class"] = _mesh([[0.1, 0.1, 0.1], [0.6, 0.2, 0.1], [0.2, 1.7, 0.3], [1.4, 1.6, 0.2], [1.5, 0.3, 0.4]],
                                       [[0, 1, 2], [1, 4, 3], [1, 3, 2]]) + (1.0,)
    C["zero_area"] = _mesh([[0.125, 0.0, 0.0], [1.125, 0.0, 0.0], [2.125, 0.0, 0.0], [3.125, 0.0, 0.0]], [[0, 1, 2], [1, 2, 3]]) + (1.0,)
    return C


CASES = _cases()
PERMUTED = ("one_triangle_three_cells", "duplicate_pair", "opposite_pair", "cube", "crease", "icosphere_0.25", "cell_boundaries",
            "non_members", "fan_257", "two_corners_one_class")


def recorded():
    """the recorded extractor output (no GPU needed): the 33^3 sphere iso-surface of tests/mesh_shells_cases.py at 2 lattice
    spacings, and the welded iso-surface with two pinched vertices of tests/mesh_fans_cases.py at 2 and 3 spacings"""
    import mesh_fans_cases
    import mesh_shells_cases
    V, T = mesh_shells_cases.extracted("sphere33")
    W, U = mesh_fans_cases.welded_lattice_touch()
    i32 = lambda t: np.ascontiguousarray(t, np.int32)
    return {"sphere33": (V, i32(T), 2.0 * float(mesh_shells_cases.SPACING)),
            "welded_touch_2": (W, i32(U), 2.0 * mesh_fans_cases.SPACING), "welded_touch_3": (W, i32(U), 3.0 * mesh_fans_cases.SPACING)}


def all_cases():
    for name, case in CASES.items():
        yield name, case
        if name in PERMUTED:
            yield name + "+permuted", permuted(case)
    yield from recorded().items()
