"""Meshes for the self-intersection tests (tests/test_mesh_intersect_*.py): name -> (verts float32 (nv, 3), tris int32 (nt, 3)).
Everything is tiny; the sphere is the closed surface of tests/ray_cases.py over the 17^3 sphere field (welded by construction)."""
import numpy as np

import mesh_shells_cases as S
import ray_cases

_mesh = S._mesh


def soup(tl):
    """triangles given as three points each, no shared indices"""
    V = np.asarray(tl, np.float64).reshape(-1, 3)
    return _mesh(V, np.arange(len(V)).reshape(-1, 3))


def shifted(mesh, by):
    return (mesh[0].astype(np.float64) + np.asarray(by, np.float64)).astype(np.float32), mesh[1]


FLOOR = [(0, 0, 0), (4, 0, 0), (0, 4, 0)]   # a triangle in the plane z = 0


def two_far():
    return soup([FLOOR, [(10, 10, 10), (11, 10, 10), (10, 11, 10.5)]])


def piercing():
    """the second triangle stands on edge through the first"""
    return soup([FLOOR, [(1, 1, -1), (1, 1, 1), (1, 3, 1)]])


def boxes_only():
    """the boxes overlap, the triangles do not meet: the second one hangs over the far corner of the first one's box"""
    return soup([FLOOR, [(3, 3, -1), (3, 3, 1), (3.5, 2.5, 0.5)]])


def folded_edge_pair():
    """two triangles on one edge, the second folded flat onto the first: adjacent, skipped"""
    return _mesh([[0, 0, 0], [4, 0, 0], [0, 4, 0], [1, 1, 0]], [[0, 1, 2], [1, 0, 3]])


def duplicate():
    return _mesh([[0, 0, 0], [4, 0, 0], [0, 4, 0]], [[0, 1, 2], [1, 2, 0]])


def vertex_pair_clear():
    """two triangles sharing vertex 0, spreading apart"""
    return _mesh([[0, 0, 0], [4, 0, 0], [0, 4, 0], [-1, -1, 3], [-3, -1, 2]], [[0, 1, 2], [0, 3, 4]])


def vertex_pair_piercing():
    """two triangles sharing vertex 0; the edge of the second opposite that vertex passes through the first"""
    return _mesh([[0, 0, 0], [4, 0, 0], [0, 4, 0], [1, 1, -1], [1, 1.5, 1]], [[0, 1, 2], [0, 3, 4]])


def coplanar_overlap():
    """both in z = 0, overlapping areas, no shared index: every segment is parallel to the other plane, nothing is reported"""
    return soup([FLOOR, [(1, 1, 0), (5, 1, 0), (1, 5, 0)]])


def t_junction():
    """a vertex of the second triangle lies on the face of the first, under its own index"""
    return soup([FLOOR, [(1, 1, 0), (1, 2, 2), (2, 1, 2)]])


def with_collapsed():
    """the piercing pair and a collapsed triangle in the middle of it"""
    V, T = piercing()
    return V, np.concatenate([T, [[0, 0, 4]]]).astype(np.int32)


def zero_area():
    """a zero-area triangle with distinct indices (three collinear points) that passes through the floor: its edges hit"""
    return soup([FLOOR, [(1, 1, -1), (1, 1, 0.5), (1, 1, 2)]])


def tetrahedron():
    return S.tetrahedron(1.0)


def cube():
    return S.cube((0, 0, 0), 1.0)


def tetrahedron_soup():
    V, T = tetrahedron()
    return _mesh(V[T].reshape(-1, 3), np.arange(12).reshape(-1, 3))


def two_tetrahedra():
    return S.join(tetrahedron(), shifted(tetrahedron(), (0.125, 0.25, 0.1875)))


def two_cubes():
    return S.join(cube(), shifted(cube(), (0.5, 0.5, 0.5)))


_sphere = {}


def sphere():
    """the closed 17^3 sphere surface -> (V, T, radius)"""
    if not _sphere:
        V, T, _, rad = ray_cases.closed_sphere(17)
        _sphere["m"] = (V, np.ascontiguousarray(T, np.int32), float(rad))
    return _sphere["m"]


def sphere17():
    return sphere()[:2]


def two_spheres():
    """the sphere and a copy translated by half a radius, in a direction that is no lattice direction"""
    V, T, rad = sphere()
    return S.join((V, T), shifted((V, T), 0.5 * rad * np.array([0.48, 0.6, 0.64])))


RANDOM_SEED = {63: 163, 64: 164, 65: 165, 200: 1200}


def random_triangles(n, offset=0.0):
    """n random triangles of edge length about 0.3 in the unit cube (a soup), translated by `offset` on every axis"""
    rng = np.random.default_rng(RANDOM_SEED[n])
    c = rng.uniform(0.15, 0.85, size=(n, 1, 3))
    P = c + rng.uniform(-0.15, 0.15, size=(n, 3, 3))
    return soup(P.astype(np.float32).astype(np.float64) + offset)


def deep():
    """150 triangles whose box centres coincide (nested sizes around one point): one Morton code, a deep tree of overlapping
    boxes"""
    rng = np.random.default_rng(15)
    tl = []
    for k in range(150):
        s = 0.5 + k / 128.0                              # (exact in float32: the box is [-s, s]^3, its centre exactly 0)
        r = rng.uniform(-0.9, 0.9, 3) * s
        tri = np.array([[-s, s, r[0]], [s, r[1], -s], [r[2], -s, s]])   # every axis reaches -s on one corner and +s on another
        tl.append(tri[:, rng.permutation(3)] * rng.choice([-1.0, 1.0], 3))
    return soup(tl)


CASES = {"empty": S.empty, "one_triangle": S.one_triangle, "two_far": two_far, "piercing": piercing, "boxes_only": boxes_only,
         "folded_edge_pair": folded_edge_pair, "duplicate": duplicate, "vertex_pair_clear": vertex_pair_clear,
         "vertex_pair_piercing": vertex_pair_piercing, "coplanar_overlap": coplanar_overlap, "t_junction": t_junction,
         "with_collapsed": with_collapsed, "zero_area": zero_area, "tetrahedron": tetrahedron, "cube": cube,
         "tetrahedron_soup": tetrahedron_soup, "two_tetrahedra": two_tetrahedra, "two_cubes": two_cubes, "sphere17": sphere17,
         "two_spheres": two_spheres, "random63": lambda: random_triangles(63), "random64": lambda: random_triangles(64),
         "random65": lambda: random_triangles(65), "random200": lambda: random_triangles(200),
         "random200_far": lambda: random_triangles(200, 1000.0), "deep": deep}
ALL = tuple(CASES)

_cases, _expected = {}, {}


def case(name):
    if name not in _cases:
        V, T = CASES[name]()
        _cases[name] = (np.ascontiguousarray(V, np.float32).reshape(-1, 3), np.ascontiguousarray(T, np.int32).reshape(-1, 3))
    return _cases[name]


def expected(name):
    """the restatement's (pairs, hits_of_tri, totals) of the case, computed once and shared"""
    if name not in _expected:
        import mesh_intersect_ref as R
        _expected[name] = R.intersections(*case(name))
        for a in _expected[name]:
            a.setflags(write=False)
    return _expected[name]
