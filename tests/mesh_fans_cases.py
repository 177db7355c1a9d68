"""Named cases for tests/test_mesh_fans_*.py (include/rho2sdf_hip.h, r2s_mesh_fans), on top of tests/mesh_shells_cases.py, whose
HAND and EXTRACTED cases are reused.  Meshes are (verts (nv, 3) float32, tris (nt, 3) int32, 0-based).  Every NEW hand case also
exists "permuted" (its triangles under a seeded shuffle) and "reversed" (a seeded 30 % of its triangles with corners 1 and 2
swapped: flipped edges still join fans).  welded_lattice_touch is an extracted surface whose field has exact zeros at lattice
points, welded with snap = 0 by tests/mesh_weld_ref.py: its triangles are recorded in tests/golden/mesh_fans_tris.npz (written by
tests/golden/make_mesh_fans_cases.py from the library's own extraction), its vertices restated by iso_ref.vertices."""
import os
import zlib

import numpy as np

import iso_ref as R
import mesh_orient_cases as O
import mesh_shells_cases as S
import mesh_weld_ref as W

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mesh_fans_tris.npz")


def _ring(n, r, z, cx=0.0):
    a = 2 * np.pi * np.arange(n) / n
    return np.stack([cx + r * np.cos(a), r * np.sin(a), np.full(n, z)], -1)


def bowtie():
    """two triangles sharing vertex 0 and nothing else: two open fans at one vertex"""
    return S._mesh([[0, 0, 0], [1, 1, 0], [1, -1, 0], [-1, 1, 0.5], [-1, -1, 0.5]], [[0, 1, 2], [0, 3, 4]])


def pinched_sphere(n=4):
    """a closed surface that touches itself in vertex 0: a cone from 0 up to ring A, a band from ring A down to ring B, a cone
    from ring B back to 0.  One shell, consistently wound, every edge regular; V - E + F = 9 - 24 + 16 = 1, and 2 (a sphere)
    once vertex 0 is split into its two fans"""
    V = np.concatenate([[[0.0, 0.0, 0.0]], _ring(n, 1.0, 1.0), _ring(n, 1.0, -1.0)])
    a, b = 1 + np.arange(n), 1 + n + np.arange(n)
    a1, b1 = np.roll(a, -1), np.roll(b, -1)
    z = np.zeros(n, np.int64)
    T = np.concatenate([np.stack([z, a, a1], -1), np.stack([a, b, b1], -1), np.stack([a, b1, a1], -1), np.stack([z, b1, b], -1)])
    return S._mesh(V, T)


def disk_and_cone(n=6):
    """vertex 0 is on the rim of a disk (an open fan of two triangles) and the apex of a cone without a base (a closed fan)"""
    rim = _ring(n, 1.0, 0.0, cx=-1.0)                 # rim[0] = (0, 0, 0) = vertex 0
    V = np.concatenate([rim, [[-1.0, 0.0, 0.0]], _ring(n, 0.5, 1.0)])
    i = np.arange(n)
    disk = np.stack([np.full(n, n), i, np.roll(i, -1)], -1)
    c = n + 1 + i
    cone = np.stack([np.zeros(n, np.int64), c, np.roll(c, -1)], -1)
    return S._mesh(V, np.concatenate([disk, cone]))


def apex300(n=300):
    """n separate triangles that share vertex 0: n open fans at one vertex; the new indices cross a block of 256"""
    rng = np.random.default_rng(3)
    V = np.concatenate([[[0.0, 0.0, 0.0]], rng.normal(size=(2 * n, 3))])
    i = np.arange(n)
    return S._mesh(V, np.stack([np.zeros(n, np.int64), 1 + 2 * i, 2 + 2 * i], -1))


def tets40(n=40):
    """n tetrahedra that share the apex 0: n closed fans of three corners at one vertex"""
    rng = np.random.default_rng(4)
    V = np.concatenate([[[0.0, 0.0, 0.0]], rng.normal(size=(3 * n, 3))])
    T = []
    for k in range(n):
        p, q, r = 1 + 3 * k, 2 + 3 * k, 3 + 3 * k
        T += [[0, q, p], [0, p, r], [0, r, q], [p, q, r]]
    return S._mesh(V, T)


def cone5000(n=5000):
    """a cone of n triangles round the apex 0 and its base, n triangles round the centre 1: two closed fans of n corners"""
    V = np.concatenate([[[0.0, 0.0, 1.0], [0.0, 0.0, 0.0]], _ring(n, 1.0, 0.0)])
    r = 2 + np.arange(n)
    r1 = np.roll(r, -1)
    return S._mesh(V, np.concatenate([np.stack([np.zeros(n, np.int64), r, r1], -1), np.stack([np.ones(n, np.int64), r1, r], -1)]))


def unused_vertices():
    """the two tetrahedra that share a vertex, with unreferenced vertices in front, between and behind"""
    V, T = S.two_tets_sharing_vertex()
    pad = np.full((1, 3), 9.0, np.float32)
    V2 = np.concatenate([pad, pad, V[:4], pad, V[4:], pad, pad, pad])
    m = np.array([2, 3, 4, 5, 7, 8, 9])
    return S._mesh(V2, m[T])


def collapsed_mixed():
    """the bowtie and a tetrahedron with collapsed triangles in between; vertex 9 is referenced by collapsed triangles only"""
    V, T = S.join(bowtie(), S.tetrahedron(1.0))
    V = np.concatenate([V, [[5.0, 5.0, 5.0]]])
    T = np.concatenate([[[9, 9, 0]], T[:1], [[0, 0, 1], [9, 5, 9]], T[1:4], [[6, 6, 6]], T[4:], [[2, 9, 2]]])
    return S._mesh(V, T)


NEW = {"bowtie": bowtie, "pinched_sphere": pinched_sphere, "disk_and_cone": disk_and_cone,
       "cubes_sharing_edge": O.two_cubes_sharing_edge, "apex300": apex300, "tets40": tets40, "cone5000": cone5000,
       "unused_vertices": unused_vertices, "collapsed_mixed": collapsed_mixed}
VARIANTS = (None, "permuted", "reversed")


# ---- the welded extracted surface ----------------------------------------------------------------------------------------------

ORIGIN, SPACING, N = (-1.0, 0.5, 0.25), 0.25, 16


def touch_field(n=N):
    """an integer-valued field of three boxes (+2 inside, -1 outside) on an n^3 lattice; A and B are one lattice step apart along
    x, B and C along y, and the lattice point between each pair has the value 0 EXACTLY: it is interior, its four lattice edges
    to the exterior cross at t = 0, so the neck between the two bodies is a ring of four coincident vertices, which the weld
    turns into one vertex with a fan on either side"""
    f = np.full((n, n, n), -1.0, np.float32)          # [z, y, x]
    f[3:8, 3:8, 2:6] = 2.0                            # A
    f[3:8, 3:8, 7:11] = 2.0                           # B
    f[3:8, 9:13, 7:11] = 2.0                          # C
    f[5, 5, 6] = 0.0                                  # between A and B
    f[4, 8, 9] = 0.0                                  # between B and C
    return f.ravel()


def fields():
    """name -> (n, flattened field) of the extracted cases (iso 0, lattice (n, n, n), ORIGIN, SPACING)"""
    return {"lattice_touch": (N, touch_field())}


def extracted(name):
    """the recorded mesh of an extracted case, as extracted (not welded)"""
    n, f = fields()[name]
    V, _ = R.vertices(f, (n, n, n), ORIGIN, SPACING, 0.0)
    with np.load(GOLDEN) as g:
        return V, g[name].astype(np.int32)


def welded_lattice_touch():
    w = W.weld(*extracted("lattice_touch"), snap=0.0)
    return S._mesh(w["verts"], w["tris"])


ALL = tuple(S.HAND) + S.EXTRACTED + tuple(NEW) + ("welded_lattice_touch",)
_cases = {}


def perm_of(name):
    """the permutation of the "permuted" variant: new triangle k is old triangle perm[k]"""
    return np.random.default_rng(zlib.crc32(name.encode()) + 1).permutation(len(case(name)[1]))


def case(name, variant=None):
    """the named mesh; variant "permuted" / "reversed" for the cases of NEW"""
    key = (name, variant)
    if key not in _cases:
        if variant is None:
            V, T = NEW[name]() if name in NEW else (welded_lattice_touch() if name == "welded_lattice_touch" else S.case(name))
        else:
            assert name in NEW and variant in VARIANTS
            V, T = case(name)
            if variant == "permuted":
                T = T[perm_of(name)]
            else:
                T = O.reverse(T, np.random.default_rng(zlib.crc32(name.encode())).random(len(T)) < 0.3)
        _cases[key] = (V, np.ascontiguousarray(T, np.int32))
    return _cases[key]


def variants():
    """every (name, variant)"""
    return [(name, None) for name in ALL] + [(name, v) for name in NEW for v in VARIANTS[1:]]
