"""Named cases of the nesting tests (tests/test_mesh_nesting_cpu.py, tests/test_mesh_nesting_gpu.py; include/rho2sdf_hip.h,
r2s_mesh_nesting).  Meshes are (verts (nv, 3) float32, tris (nt, 3) int32, 0-based).

case(name) -> (V, T); built(name) -> the expectation a CONSTRUCTED case carries from how it was put together, independent of any
ray: patch_of_tri (nt,), closed (n,) bool and containers, one set of patch numbers per patch.  forest(containers) turns that
into depth, parent and irregular by the header's definition.  The coordinates of the constructed cases are small dyadic numbers
(the icosphere apart), so every operation of the pair test is exact on them and a ray through a vertex or along an edge is
decided by the tie rule alone.  The extracted cases are iso-surfaces on small lattices; their triangles are recorded in
tests/golden/mesh_nesting_tris.npz (tests/golden/make_mesh_nesting_cases.py), their vertices restated by iso_ref.vertices."""
import os

import numpy as np

import iso_ref as R
import mesh_holes_cases as H
import mesh_orient_cases as O
import mesh_shells_cases as S
import mesh_winding_cases as W

ORIGIN, SPACING = (-1.0, 0.5, 0.25), 0.25
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mesh_nesting_tris.npz")


def _built(parts, containers, closed=None):
    """parts: meshes that are one patch each, in patch order"""
    V, T = S.join(*parts)
    pot = np.concatenate([np.full(len(t), k, np.int32) for k, (_, t) in enumerate(parts)])
    closed = [True] * len(parts) if closed is None else closed
    return V, T, dict(patch_of_tri=pot, closed=np.array(closed, bool), containers=[set(c) for c in containers])


def tet(c, L):
    V, T = S.tetrahedron(L)
    return (V.astype(np.float64) + np.asarray(c, np.float64)).astype(np.float32), T


def beside():
    """the -x ray from the small cube's sample crosses the big cube twice: an even count, no containment"""
    return _built([S.cube((0, 0, 0), 1.0), S.cube((3, 0.25, 0.25), 0.5)], [(), ()])


def nested2():
    return _built([S.cube((0, 0, 0), 4.0), S.cube((1, 1.5, 1.25), 1.0)], [(), (0,)])


def chain3():
    return _built([S.cube((0, 0, 0), 8.0), S.cube((1, 1.5, 2), 4.0), S.cube((2, 2.5, 3), 1.0)], [(), (0,), (0, 1)])


def siblings():
    return _built([S.cube((0, 0, 0), 8.0), S.cube((1, 1, 1.5), 2.0), S.cube((5, 4, 3), 2.0)], [(), (0,), (0,)])


def void_island():
    """a void wound inward with an island inside it: the windings play no part"""
    return _built([S.cube((0, 0, 0), 8.0), S.cube((1, 1, 1), 5.0, reverse=True), S.cube((2, 3, 2.5), 1.0)], [(), (0,), (0, 1)])


def open_query():
    """a lone triangle inside a cube: an open patch is a query"""
    tri = S._mesh([[1, 1, 1], [2, 1, 1.5], [1, 2, 1.25]], [[0, 1, 2]])
    return _built([S.cube((0, 0, 0), 4.0), tri], [(), (0,)], [True, False])


def open_container():
    """a small cube inside a cube without one face: an open surface is no container"""
    return _built([H.cube_minus_face((0.0, 0.0, 0.0), 4.0), S.cube((1, 1.5, 1.25), 1.0)], [(), ()], [False, True])


def shared_edge():
    """two welded unit cubes sharing an edge (four half-edges in one group: neither is closed) around a small cube"""
    V, T = S.join(O.two_cubes_sharing_edge(), S.cube((0.25, 0.5, 0.25), 0.25))
    pot = np.repeat(np.arange(3, dtype=np.int32), 12)
    return V, T, dict(patch_of_tri=pot, closed=np.array([False, False, True]), containers=[set(), set(), set()])


def collapsed_mixed():
    V, T, e = nested2()
    col = np.array([[0, 0, 1]], np.int32)
    T = np.concatenate([col, T[:5], col + 3, T[5:12], col, T[12:], col + 9])
    pot = np.concatenate([[-1], e["patch_of_tri"][:5], [-1], e["patch_of_tri"][5:12], [-1], e["patch_of_tri"][12:], [-1]]).astype(np.int32)
    return V, T, dict(e, patch_of_tri=pot)


def through_octa():
    """the six axis rays from the inner sample (0.5, 0, 0) leave through vertices and edges of the outer octahedron"""
    return _built([W.octahedron(2.0), W.octahedron(0.5)], [(), (0,)])


def through_cube_vertices():
    """the sample (0, 0, 0): every axis ray leaves through the centre vertex of a face of 2 x 2 quads"""
    return _built([W.box_mesh(-2, 2, 2), S.cube((0, 0, 0), 1.0)], [(), (0,)])


def through_cube_edges():
    """the sample (-0.5, -0.5, -0.5): every axis ray leaves through the diagonal edge of a quad"""
    return _built([W.box_mesh(-2, 2, 2), S.cube((-0.5, -0.5, -0.5), 1.0)], [(), (0,)])


def interpenetrating():
    """a cube pierced by a beam, no vertex of either inside the other, and a tetrahedron in the intersection: depth 2 with both
    containers at depth 0 - the parent by the tie rule (the smaller number), and irregular"""
    return _built([S.cube((0, 0, 0), 4.0), W.box_mesh((1, 1, -1), (3, 3, 5), 1), tet((1.5, 1.25, 1), 1.0)], [(), (), (0, 1)])


def chain70():
    """70 nested cubes (840 triangles): depth 69, more containers than a wavefront has lanes"""
    parts = [S.cube((k / 4, k / 8, 3 * k / 16), 40.0 - k / 2) for k in range(70)]
    return _built(parts, [tuple(range(k)) for k in range(70)])


def scatter(n):
    """n small tetrahedra at seeded dyadic positions outside, between and inside two nested cubes"""
    rng = np.random.default_rng(n)
    zones = []
    for z, (lo, hi) in enumerate((((18, 0, 0), (30, 16, 16)), ((0.5, 0.5, 0.5), (3, 15, 15)), ((5, 5, 5), (11, 11, 11)))):
        g = [np.arange(lo[k], hi[k], 0.5) for k in range(3)]
        cells = np.stack(np.meshgrid(*g, indexing="ij"), -1).reshape(-1, 3)
        zones.append((z, cells))
    parts, cont = [S.cube((0, 0, 0), 16.0), S.cube((4, 4, 4), 8.0)], [(), (0,)]
    which = rng.integers(0, 3, n)
    for k in range(n):
        z, cells = zones[which[k]]
        c = cells[rng.integers(0, len(cells))] + rng.integers(0, 16, 3) / 64.0
        zones[which[k]] = (z, cells[(cells != np.floor(c * 2) / 2).any(1)])          # a cell holds one tetrahedron
        parts.append(tet(c, 0.125))
        cont.append(((), (0,), (0, 1))[z])
    return _built(parts, cont)


def ico_around():
    """an icosphere of 5 120 triangles (radius 4) around 40 small tetrahedra"""
    Vi, Ti = H.icosphere(4)
    rng = np.random.default_rng(40)
    cells = np.stack(np.meshgrid(*[np.arange(-2.0, 2.0, 0.5)] * 3, indexing="ij"), -1).reshape(-1, 3)
    pick = rng.choice(len(cells), 40, replace=False)
    parts = [((Vi.astype(np.float64) * 4.0).astype(np.float32), Ti)]
    parts += [tet(cells[i] + rng.integers(0, 16, 3) / 64.0, 0.125) for i in pick]
    return _built(parts, [()] + [(0,)] * 40)


BUILT = {"one_triangle": lambda: _built([S.one_triangle()], [()], [False]), "tetrahedron": lambda: _built([S.tetrahedron(1.0)], [()]),
         "beside": beside, "nested2": nested2, "chain3": chain3, "siblings": siblings, "void_island": void_island,
         "open_query": open_query, "open_container": open_container, "shared_edge": shared_edge, "collapsed_mixed": collapsed_mixed,
         "through_octa": through_octa, "through_cube_vertices": through_cube_vertices, "through_cube_edges": through_cube_edges,
         "interpenetrating": interpenetrating, "chain70": chain70, "scatter255": lambda: scatter(255), "scatter256": lambda: scatter(256),
         "scatter257": lambda: scatter(257), "ico_around": ico_around}
EXTRACTED = ("hollow21", "noise17")
ALL = ("empty",) + tuple(BUILT) + EXTRACTED


def hollow_field(n=21):
    """a ball of radius 8 with a concentric hollow of radius 4 on an n^3 lattice of unit spacing"""
    g = np.arange(n, dtype=np.float64)
    c = (n - 1) / 2
    z, y, x = np.meshgrid(g, g, g, indexing="ij")
    d = np.sqrt((x - c) ** 2 + (y - c) ** 2 + (z - c) ** 2)
    return np.minimum(8.0 - d, d - 4.0).astype(np.float32).ravel()


def fields():
    """name -> (n, flattened field) of the extracted cases (iso 0, lattice (n, n, n), ORIGIN, SPACING)"""
    return {"hollow21": (21, hollow_field()), "noise17": (17, S.noise_field(17, seed=9))}


_cases = {}


def _case(name):
    if name not in _cases:
        if name == "empty":
            _cases[name] = S.empty() + (dict(patch_of_tri=np.zeros(0, np.int32), closed=np.zeros(0, bool), containers=[]),)
        elif name in BUILT:
            _cases[name] = BUILT[name]()
        else:
            n, f = fields()[name]
            V, _ = R.vertices(f, (n, n, n), ORIGIN, SPACING, 0.0)
            with np.load(GOLDEN) as g:
                _cases[name] = (V, g[name].astype(np.int32), None)
    return _cases[name]


def case(name):
    return _case(name)[:2]


def built(name):
    return _case(name)[2]


def forest(containers):
    """depth, parent, irregular of the header's definition from the containers of every patch"""
    n = len(containers)
    depth = np.array([len(c) for c in containers], np.int64).reshape(n)
    parent = np.array([max(c, key=lambda q: (depth[q], -q)) if c else -1 for c in containers], np.int64).reshape(n)
    irregular = np.array([depth[p] > 0 and depth[parent[p]] != depth[p] - 1 for p in range(n)], bool).reshape(n)
    return depth, parent, irregular


def reversed_some(T, seed=30, share=0.3):
    """T with a seeded 30 % of the triangles reversed, (i0, i1, i2) -> (i0, i2, i1): the sample of every patch stays"""
    T = T.copy()
    sel = np.random.default_rng(seed).random(len(T)) < share
    T[sel] = T[sel][:, [0, 2, 1]]
    return T
