"""Named cases for tests/test_mesh_holes_*.py (include/rho2sdf_hip.h, r2s_mesh_holes), on top of tests/mesh_shells_cases.py and
tests/mesh_orient_cases.py.  Meshes are (verts (nv, 3) float32, tris (nt, 3) int32, 0-based), all built in numpy; the two recorded
iso-surfaces come from tests/golden/mesh_shells_tris.npz.  Every case with a closed rim of more than 3 edges (VARIED) also exists
"permuted" (its triangles under a seeded shuffle) and "rotated" (every triangle's corners rotated by a seeded 0, 1 or 2 places:
the same triangles and windings under other half-edge ids)."""
import zlib

import numpy as np

import mesh_orient_cases as O
import mesh_shells_cases as S


def cube_minus_face(lo=(0.0, 0.0, 0.0), side=1.0):
    """the cube without the two triangles of its face z = lo_z: one rim of 4 edges; the fill puts w at the face centre"""
    V, T = S.cube(lo, side)
    return V, np.ascontiguousarray(T[2:])


def cube_far():
    """the same cube scaled to 0.1 and moved to 1000: the reference point keeps the sums small"""
    return cube_minus_face((1000.0, 1000.0, 1000.0), 0.1)


def tet_minus_face():
    V, T = S.tetrahedron(1.0)
    return V, np.ascontiguousarray(T[:3])


def tube(n=8, z0=3.0):
    """an open tube of n quads round the z axis: two rims of n edges"""
    a = 2 * np.pi * np.arange(n) / n
    ring = lambda z: np.stack([5.0 + np.cos(a), np.sin(a), np.full(n, z)], -1)   # noqa: E731
    V = np.concatenate([ring(z0), ring(z0 + 1.0)])
    i = np.arange(n)
    j = np.roll(i, -1)
    T = np.concatenate([np.stack([i, j, n + j], -1), np.stack([i, n + j, n + i], -1)])
    return S._mesh(V, T)


def tube_and_cube():
    return S.join(tube(), cube_minus_face())


def loops_and_chain():
    """closed rims of 3, 4, 5 and twice 300 edges (9 rounds of pointer jumping, each across a block edge of the sums) next to the
    open chain of the fin"""
    return S.join(tube(300), tet_minus_face(), cube_minus_face(), disk(5), fin())


def bowtie():
    """two triangles sharing vertex 0 and nothing else: one rim of 6 edges through a branch node; two rims of 3 after the split"""
    return S._mesh([[0, 0, 0], [1, 1, 0], [1, -1, 0], [-1, 1, 0.5], [-1, -1, 0.5]], [[0, 1, 2], [0, 3, 4]])


def icosphere(level):
    t = (1.0 + 5.0 ** 0.5) / 2.0
    V = [[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t], [t, 0, -1], [t, 0, 1],
         [-t, 0, -1], [-t, 0, 1]]
    T = [[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6], [7, 1, 8],
         [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]]
    V = [np.array(p, np.float64) / np.linalg.norm(p) for p in V]
    for _ in range(level):
        mid, T2 = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                p = V[a] + V[b]
                V.append(p / np.linalg.norm(p))
                mid[k] = len(V) - 1
            return mid[k]
        for a, b, c in T:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            T2 += [[a, ab, ca], [b, bc, ab], [c, ca, bc], [ab, bc, ca]]
        T = T2
    return S._mesh(np.array(V), T)


def ico_touching_holes():
    """an icosphere of 320 triangles without two triangles that share exactly one vertex: the two holes touch in a branch node,
    one rim of 6 edges that is not closed; the fans' split turns it into one closed rim of 6"""
    V, T = icosphere(2)
    rows = T.tolist()
    for j in range(1, len(rows)):
        if len(set(rows[0]) & set(rows[j])) == 1:
            return V, np.ascontiguousarray(np.delete(T, [0, j], 0))
    raise AssertionError


def strip_one_reversed():
    """a strip of 8 triangles with triangle 3 reversed: flipped nodes where its boundary edge meets its neighbours'"""
    V, T = S.ribbon(8)
    return V, O.reverse(T, [3])


def fin():
    """a tetrahedron with a fin on its edge {0, 1}: the edge is non-manifold, the fin's two other edges are a chain with two open
    nodes"""
    V, T = S.tetrahedron(1.0)
    return S._mesh(np.concatenate([V, [[0.5, -1.0, -1.0]]]), np.concatenate([T, [[0, 1, 4]]]))


def degenerate_mixed():
    """the cube without a face, with collapsed triangles in between and unused vertices in front and behind; vertex 9 is
    referenced by collapsed triangles only"""
    V, T = cube_minus_face()
    pad = np.full((1, 3), 9.0, np.float32)
    V2 = np.concatenate([pad, V, pad, pad])
    T2 = T + 1
    T2 = np.concatenate([[[9, 9, 1]], T2[:3], [[1, 1, 2], [9, 3, 9]], T2[3:], [[4, 4, 4]]])
    return S._mesh(V2, T2)


def disk(n):
    """n triangles round a centre: one rim of n edges (the centre is the LAST vertex, the rim runs 0 -> 1 -> .. -> n - 1)"""
    a = 2 * np.pi * np.arange(n) / n
    V = np.concatenate([np.stack([2.0 + np.cos(a), np.sin(a) - 1.0, 0.2 * np.sin(3 * a)], -1), [[2.0, -1.0, 0.5]]])
    i = np.arange(n)
    return S._mesh(V, np.stack([np.full(n, n), i, np.roll(i, -1)], -1))


def _delete_isolated(T, n_tris, n_stars, seed):
    """T without n_tris single triangles and n_stars whole vertex stars, no two of the deleted patches sharing a vertex"""
    rng = np.random.default_rng(seed)
    nv = int(T.max()) + 1
    star = [[] for _ in range(nv)]
    for ti, tri in enumerate(T.tolist()):
        for q in tri:
            star[q].append(ti)
    blocked, gone = np.zeros(nv, bool), []
    for vert in rng.permutation(nv).tolist():
        if n_stars == 0:
            break
        ring = np.unique(T[star[vert]])
        if not blocked[ring].any():
            gone += star[vert]
            blocked[np.unique(T[[t for q in ring for t in star[q]]])] = True
            n_stars -= 1
    for ti in rng.permutation(len(T)).tolist():
        if n_tris == 0:
            break
        if not blocked[T[ti]].any():
            gone.append(ti)
            blocked[np.unique(T[[t for q in T[ti] for t in star[q]]])] = True
            n_tris -= 1
    assert n_tris == 0 and n_stars == 0
    return np.ascontiguousarray(np.delete(T, gone, 0))


def ico_many_holes():
    """an icosphere of 20 480 triangles with 200 isolated triangles and 50 vertex stars deleted: 250 closed rims of 3, 5 or 6 edges"""
    V, T = icosphere(5)
    return V, _delete_isolated(T, 200, 50, 7)


def sphere33_holes():
    """the recorded iso-surface sphere33 with 30 isolated triangles and 10 vertex stars deleted"""
    V, T = S.extracted("sphere33")
    return V, _delete_isolated(T, 30, 10, 8)


HAND = {"empty": S.empty, "one_triangle": S.one_triangle, "all_collapsed": S.all_collapsed, "tetrahedron": lambda: S.tetrahedron(1.0),
        "tet_minus_face": tet_minus_face, "cube_minus_face": cube_minus_face, "cube_far": cube_far, "tube_and_cube": tube_and_cube,
        "bowtie": bowtie, "ico_touching_holes": ico_touching_holes, "strip_one_reversed": strip_one_reversed, "moebius": O.moebius,
        "fin": fin, "three_on_edge": S.three_on_edge, "degenerate_mixed": degenerate_mixed, "disk255": lambda: disk(255),
        "disk256": lambda: disk(256), "disk257": lambda: disk(257), "disk16385": lambda: disk(16385), "ico_many_holes": ico_many_holes,
        "sphere33_holes": sphere33_holes, "gyroid17": lambda: S.extracted("gyroid17"), "loops_and_chain": loops_and_chain}
VARIED = ("cube_minus_face", "cube_far", "tube_and_cube", "degenerate_mixed", "disk255", "disk256", "disk257", "disk16385",
          "ico_many_holes", "sphere33_holes", "gyroid17", "loops_and_chain")
VARIANTS = (None, "permuted", "rotated")
ALL = tuple(HAND)
_cases = {}


def perm_of(name):
    """the permutation of the "permuted" variant: new triangle k is old triangle perm[k]"""
    return np.random.default_rng(zlib.crc32(name.encode()) + 1).permutation(len(case(name)[1]))


def rot_of(name):
    """the rotations of the "rotated" variant: new corner c of triangle k is old corner (c + rot[k]) % 3"""
    return np.random.default_rng(zlib.crc32(name.encode()) + 2).integers(0, 3, len(case(name)[1]))


def old_half_edge(name, variant, h):
    """the half-edge ids h of a variant as ids of the plain case"""
    h = np.asarray(h, np.int64)
    if variant is None:
        return h
    if variant == "permuted":
        return 3 * perm_of(name)[h // 3] + h % 3
    return 3 * (h // 3) + (h % 3 + rot_of(name)[h // 3]) % 3


def case(name, variant=None):
    key = (name, variant)
    if key not in _cases:
        if variant is None:
            V, T = HAND[name]()
        else:
            assert name in VARIED and variant in VARIANTS
            V, T = case(name)
            if variant == "permuted":
                T = T[perm_of(name)]
            else:
                T = T[np.arange(len(T))[:, None], (np.arange(3)[None, :] + rot_of(name)[:, None]) % 3]
        _cases[key] = (V, np.ascontiguousarray(T, np.int32))
    return _cases[key]


def variants():
    """every (name, variant)"""
    return [(name, None) for name in ALL] + [(name, v) for name in VARIED for v in VARIANTS[1:]]


FILLS = (-1, 0, 4, 8)   # the max_edges the tests ask for
