"""Named cases for tests/test_mesh_orient_*.py (include/rho2sdf_hip.h, r2s_mesh_orient), on top of tests/mesh_shells_cases.py.
Meshes are (verts (nv, 3) float32, tris (nt, 3) int32, 0-based).  Every case also exists SCRAMBLED: a seeded random 30 % of its
triangles get corners 1 and 2 swapped."""
import zlib

import numpy as np

import mesh_shells_cases as S


def reverse(T, which=None):
    """T with corners 1 and 2 swapped in the rows `which` (None: all)"""
    T = np.array(T, np.int32)
    which = slice(None) if which is None else which
    T[which] = T[which][:, [0, 2, 1]]
    return T


def tetrahedron_reversed():
    V, T = S.tetrahedron()
    return V, reverse(T)


def tetrahedron_one_reversed():
    V, T = S.tetrahedron()
    return V, reverse(T, [2])


def two_same_direction():
    """two triangles that both run 0 -> 1 along their shared edge: one flipped edge, a majority tie"""
    return S._mesh([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, -1, 0.5]], [[0, 1, 2], [0, 1, 3]])


def two_cubes_sharing_edge():
    """unit cubes at (0, 0, 0) and (1, 1, 0) that share the edge x = y = 1 through common vertex indices: four half-edges in
    one group, so nothing is joined across it - each cube is its own patch, and neither is closed"""
    V, T = S.join(S.cube((0, 0, 0), 1.0), S.cube((1, 1, 0), 1.0))
    T = T.copy()
    T[T == 8], T[T == 12] = 3, 7          # the second cube's corners (1, 1, 0) and (1, 1, 1) are the first cube's 3 and 7
    return V, T


def moebius(n=9):
    """a Moebius strip of n quads, two triangles each; the last quad closes onto the first with the rims exchanged"""
    k = np.arange(n)
    u = 2 * np.pi * k / n
    V = np.empty((2 * n, 3))
    for s, v in ((0, -0.3), (1, 0.3)):
        V[s::2] = np.stack([(1 + v * np.cos(u / 2)) * np.cos(u), (1 + v * np.cos(u / 2)) * np.sin(u), v * np.sin(u / 2)], -1)
    T = []
    for i in range(n):
        a, b = 2 * i, 2 * i + 1
        a1, b1 = (2 * i + 2, 2 * i + 3) if i < n - 1 else (1, 0)
        T += [[a, a1, b1], [a, b1, b]]
    return S._mesh(V, T)


def moebius_and_tetrahedron():
    V, T = S.tetrahedron(1.0)
    return S.join(moebius(), (V + np.float32(3.0), T))


def ribbon_alternating(n=3000):
    """the strip of n triangles with every second triangle reversed: union chains across workgroups, a majority tie"""
    V, T = S.ribbon(n)
    return V, reverse(T, np.arange(1, n, 2))


def _first(mesh, n):
    """the mesh with its first n triangles only"""
    return mesh[0], mesh[1][:n]


def ribbon_alternating_shuffled():
    return S.permuted(ribbon_alternating(), 21)[0]


HAND = {"empty": S.empty, "one_triangle": S.one_triangle, "all_collapsed": S.all_collapsed, "tetrahedron": S.tetrahedron,
        "tetrahedron_reversed": tetrahedron_reversed, "tetrahedron_one_reversed": tetrahedron_one_reversed,
        "cube_one_reversed": S.cube_one_reversed, "cube_with_void": S.cube_with_void, "two_same_direction": two_same_direction,
        "triangle_twice": S.triangle_twice, "three_on_edge": S.three_on_edge, "fans40": lambda: S.fans(40),
        "two_cubes_sharing_edge": two_cubes_sharing_edge, "two_tets_sharing_vertex": S.two_tets_sharing_vertex, "moebius": moebius,
        "moebius_and_tetrahedron": moebius_and_tetrahedron, "ribbon_alternating": ribbon_alternating,
        "ribbon_alternating_shuffled": ribbon_alternating_shuffled, "disjoint": lambda: S.disjoint(3000),
        "torus": lambda: S.torus(100, 100)}
EXTRACTED = ("sphere33", "nested41")
ALL = tuple(HAND) + EXTRACTED
# one patch of 65 blocks of 256 sorted triangles (the first with two block partials per lane of the combine) and one of 129
# blocks (the last lane's run is short): named for tests/test_mesh_segsum_gpu.py, too long for the plain-Python restatement of
# every test that walks ALL
LONG = {"ribbon16385": lambda: _first(ribbon_alternating(16386), 16385),
        "ribbon32769": lambda: _first(ribbon_alternating(32770), 32769)}
TIE_FREE = ("cube_one_reversed", "moebius_and_tetrahedron", "torus", "nested41")   # (their scrambled copies too)

_cases = {}


def case(name, scrambled=False):
    """the named mesh; scrambled: a seeded random 30 % of its triangles have corners 1 and 2 swapped"""
    key = (name, bool(scrambled))
    if key not in _cases:
        V, T = HAND[name]() if name in HAND else LONG[name]() if name in LONG else S.extracted(name)
        if scrambled:
            pick = np.random.default_rng(zlib.crc32(name.encode())).random(len(T)) < 0.3
            T = reverse(T, pick)
        _cases[key] = (V, np.ascontiguousarray(T, np.int32))
    return _cases[key]


def variants():
    """every (name, scrambled)"""
    return [(name, s) for name in ALL for s in (False, True)]
