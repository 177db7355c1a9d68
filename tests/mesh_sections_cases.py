"""Case generators for tests/test_mesh_sections_*.py (include/rho2sdf_hip.h, r2s_mesh_sections).  A case is
(verts (nv, 3) float32, tris (nt, 3) int32, normal (3,) float64, levels (n,) float64).  The meshes are those of
mesh_shells_cases (the extracted ones from its recorded tests/golden/mesh_shells_tris.npz) and a few built here; the levels
are chosen so that each case reaches one way the kernels can go wrong (the table in the docstring of
tests/test_mesh_sections_gpu.py)."""
import numpy as np

import mesh_holes_cases as H
import mesh_shells_cases as S

Z = (0.0, 0.0, 1.0)


def _case(mesh, normal, levels):
    V, T = mesh
    return V, T, np.asarray(normal, np.float64), np.asarray(levels, np.float64).reshape(-1)


def band(n=20000):
    """S.ribbon's strip of n triangles closed into a band around the z axis: a lower and an upper rim of n / 2 vertices each,
    triangle t shares an edge with t - 1 and t + 1 (cyclically).  The plane z = 0 cuts every triangle: one loop of n segments"""
    m = n // 2
    a = 2 * np.pi * np.arange(m) / m
    V = np.empty((2 * m, 3))
    V[0::2] = np.stack([np.cos(a), np.sin(a), -0.5 + 0.05 * np.sin(3 * a)], -1)
    V[1::2] = np.stack([(1 + 0.1 * np.cos(5 * a)) * np.cos(a), (1 + 0.1 * np.cos(5 * a)) * np.sin(a), 0.5 + 0.05 * np.cos(2 * a)], -1)
    q = 2 * np.arange(m)
    w = 2 * m
    T = np.stack([np.stack([q, (q + 2) % w, q + 1], -1), np.stack([q + 1, (q + 2) % w, (q + 3) % w], -1)], 1).reshape(-1, 3)
    return S._mesh(V, T)


def cone(m, centre=(0.0, 0.0)):
    """m triangles from an apex at z = -1 to a rim of m vertices at z = 1: any plane between cuts a loop of m segments"""
    a = 2 * np.pi * np.arange(m) / m
    rim = np.stack([centre[0] + np.cos(a), centre[1] + np.sin(a), np.ones(m)], -1)
    V = np.concatenate([[[centre[0], centre[1], -1.0]], rim])
    i = np.arange(m)
    return S._mesh(V, np.stack([np.zeros(m, int), 1 + (i + 1) % m, 1 + i], -1))


LOOP_SIZES = (3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 33, 63, 64, 65, 127, 129, 255, 256, 257, 511, 513, 1023, 1025)


def cones():
    """one cone per loop size, side by side, cut by two planes: loops that end at, before and behind the block edges of the
    sums and the powers of two of pointer jumping; the triangles shuffled so that no loop is in segment order"""
    mesh = S.join(*[cone(m, (3.0 * k, 0.0)) for k, m in enumerate(LOOP_SIZES)])
    return S.permuted(mesh, 7)[0]


def loops_and_chain():
    """cones of 3, 4 and 5 triangles, an open tube of 300 and a single triangle, cut by one plane: closed loops of 3, 4, 5 and
    300 segments (9 rounds of pointer jumping, across a block edge of the sums) next to an open chain"""
    mesh = S.join(cone(3), cone(4, (3.0, 0.0)), cone(5, (6.0, 0.0)), H.tube(150, -0.5), S.one_triangle())
    return _case(mesh, Z, [0.125])


def stacked_cubes():
    """two cubes of side 8 stacked along z at (-2^20, 2^20, 2^20) (the double spacing of a coordinate there is 2^-32), normal
    (1, 0, 1): the heights x + z are small integers, exact, so two levels that are neighbouring doubles (2^-50 apart) give
    points whose coordinates differ by far less than their spacing: both contours of a cube have bit-equal points, and only
    the level tells their nodes apart"""
    b = 2.0 ** 20
    mesh = S.join(S.cube((-b, b, b), 8.0), S.cube((-b, b, b + 8.0), 8.0))
    return _case(mesh, (1.0, 0.0, 1.0), [4.0, np.nextafter(4.0, np.inf), 20.0, np.nextafter(20.0, np.inf)])


def _lattice_levels(n):
    """one level per lattice plane of the extracted cases along z and one halfway between"""
    return S.ORIGIN[2] + 0.5 * S.SPACING * np.arange(2 * n - 1)


def _torus_saddle():
    V, T = S.torus()
    # (1, 0, 0): h is x exactly; x = 1.3 is the saddle vertex on the inner equator, 2.7 the outermost vertex
    return _case((V, T), (1.0, 0.0, 0.0), [float(np.float32(1.3)), float(V[:, 0].max())])


HAND = {
    "empty": lambda: _case(S.empty(), Z, [0.0, 1.0]),
    "no_levels": lambda: _case(S.cube((0, 0, 0), 1.0), Z, []),
    "levels_outside": lambda: _case(S.cube((0, 0, 0), 1.0), Z, [-3.0, -2.0, 1.5, 7.0]),
    "all_collapsed": lambda: _case(S.all_collapsed(), Z, [0.0]),
    "one_triangle": lambda: _case(S.one_triangle(), Z, [0.125, 0.25]),
    "three_on_edge": lambda: _case(S.three_on_edge(), (1.0, 0.0, 0.0), [0.25, 0.5]),
    "triangle_twice": lambda: _case(S.triangle_twice(), Z, [0.25]),
    "cube_one_reversed": lambda: _case(S.cube_one_reversed(), Z, [0.5, 1.0]),
    "cube_with_void": lambda: _case(S.cube_with_void(), Z, [0.25, 1.0, 1.75]),
    "cube_bottom": lambda: _case(S.cube((0, 0, 0), 1.5), Z, [0.0]),
    "cube_top": lambda: _case(S.cube((0, 0, 0), 1.5), Z, [1.5]),
    "stacked_cubes": stacked_cubes,
    "tet_integer_levels": lambda: _case(S.tetrahedron(), Z, np.arange(1.0, 60.0)),
    "tet_1000_levels": lambda: _case(S.tetrahedron(), (1.0, 2.0, 3.0), 180.0 * (np.arange(1000) + 0.5) / 1000),
    "tet_vertex_levels_z": lambda: _case(S.tetrahedron(), Z, [0.0, 60.0]),
    "tet_vertex_levels_111": lambda: _case(S.tetrahedron(), (1.0, 1.0, 1.0), [0.0, 60.0]),
    "torus_saddle": _torus_saddle,
    "torus_123": lambda: _case(S.torus(), (1.0, 2.0, 3.0), [-2.5, -0.4, 0.0, 0.3, 1.1, 4.0]),
    "band20000": lambda: _case(band(), Z, [0.0]),
    "cones": lambda: _case(cones(), Z, [-0.5, 0.25]),
    "loops_and_chain": loops_and_chain,
}
EXTRACTED = ("sphere33", "gyroid17", "noise24_closed", "noise24_open")
ALL = tuple(HAND) + EXTRACTED

_cases = {}


def case(name):
    if name not in _cases:
        if name in HAND:
            _cases[name] = HAND[name]()
        else:
            n = S.fields()[name][0]
            _cases[name] = _case(S.case(name), Z, _lattice_levels(n))
    return _cases[name]


def permuted(c, seed):
    """(case with its triangles under a seeded shuffle, perm): new triangle k is old triangle perm[k]"""
    V, T, normal, levels = c
    (_, Tp), perm = S.permuted((V, T), seed)
    return (V, Tp, normal, levels), perm
