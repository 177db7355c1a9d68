"""Case generators for tests/test_mesh_weld_*.py (include/rho2sdf_hip.h, r2s_mesh_weld).  A case is (verts (nv, 3) float32,
tris (nt, 3) int32 0-based or None for a soup, snap): `snap` is the positive cell size the case is ALSO run with (every case
runs with snap = 0 as well).  Each case aims at one way the kernels can go wrong."""
import numpy as np

import mesh_shells_cases as S


def _v(V):
    return np.asarray(V, np.float32).reshape(-1, 3)


def _t(T):
    return np.asarray(T, np.int32).reshape(-1, 3)


def empty():
    return _v([]), None, 0.5


def no_tris():
    """vertices, some of them equal, and an indexed mesh without a triangle: every class is unused"""
    return _v([[0, 0, 0], [1, 2, 3], [0, 0, 0], [1, 2, 3], [4, 5, 6]]), _t([]), 0.5


def one_triangle():
    return _v([[0, 0, 0], [1, 0, 0], [0, 1, 0.5]]), None, 0.25


def all_one_point():
    """300 vertices at one coordinate: one run longer than a 256-thread block; all 100 soup triangles collapse"""
    return np.tile(_v([[0.3, -1.7, 2.5]]), (300, 1)), None, 0.125


def signed_zero():
    """-0.0 and +0.0 merge in each axis; the first one's bits are kept (vertices 0, 2 and 4 are the -0.0 ones)"""
    n, p = np.float32(-0.0), np.float32(0.0)
    V = _v([[n, 1, 2], [p, 1, 2], [3, n, 4], [3, p, 4], [5, 6, n], [5, 6, p], [p, p, p], [n, n, n], [7, 7, 7]])
    return V, _t([[0, 2, 4], [1, 3, 5], [6, 7, 8]]), 0.5


def denormal_and_huge():
    """denormals are ordinary values (two different ones stay apart, equal ones merge, none equals 0) next to the largest
    finite float32; with snap = 2^100 the huge values fall into cells near +-2^28 and the denormals into cells 0 and -1"""
    d1, d2 = np.float32(1e-45), np.float32(3e-45)        # (the two smallest denormals that differ)
    h = np.finfo(np.float32).max
    V = _v([[d1, 0, 0], [d2, 0, 0], [d1, 0, 0], [0, 0, 0], [-d1, 0, 0], [h, -h, h], [h, -h, h], [h, h, -h],
            [np.float32(1.17549435e-38), d2, -d2]])
    return V, _t([[0, 1, 3], [2, 1, 4], [5, 6, 7], [3, 7, 8]]), float(2.0 ** 100)


def differ_in_one_axis():
    """triples equal in two words and different in the third, for each axis, interleaved with exact repeats: a sort that drops or
    misorders one word merges or splits them"""
    base = [[1, 2, 3], [9, 2, 3], [1, 9, 3], [1, 2, 9], [1, 2, 3], [9, 2, 3], [1, 9, 3], [1, 2, 9], [2, 1, 3], [3, 2, 1], [1, 3, 2]]
    V = _v(base)
    T = _t([[0, 1, 2], [4, 5, 6], [3, 7, 8], [8, 9, 10], [0, 4, 3]])
    return V, T, 4.0


def runs_across_blocks():
    """1 000 vertices in classes of size 1..9, shuffled, so the sorted runs straddle the borders of the 256-thread blocks"""
    rng = np.random.default_rng(11)
    pts, sizes = [], []
    while sum(sizes) < 1000:
        sizes.append(min(1 + len(sizes) % 9, 1000 - sum(sizes)))
    for s in sizes:
        pts += [rng.integers(-50, 50, 3).astype(np.float32) * np.float32(0.37)] * s
    V = _v(pts)[rng.permutation(1000)]
    T = rng.integers(0, 1000, (700, 3)).astype(np.int32)
    return V, T, 1.0


_CUBE_V = [[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0, 0, 1], [1, 0, 1], [1, 1, 1], [0, 1, 1]]
_CUBE_T = [[0, 2, 1], [0, 3, 2], [4, 5, 6], [4, 6, 7], [0, 1, 5], [0, 5, 4], [1, 2, 6], [1, 6, 5], [2, 3, 7], [2, 7, 6], [3, 0, 4],
           [3, 4, 7]]


def cube_soup():
    """12 triangles, 36 vertices welding to 8"""
    return _v(_CUBE_V)[np.array(_CUBE_T).ravel()], None, 0.5


def rotations():
    """(a,b,c), (b,c,a), (c,a,b) are duplicates; (a,c,b) is the opposite orientation; a second class with only one orientation
    twice and a third with both orientations twice"""
    V = _v([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 1]])
    T = _t([[0, 1, 2], [1, 2, 0], [2, 0, 1], [0, 2, 1], [1, 3, 2], [3, 2, 1], [4, 3, 0], [3, 4, 0], [0, 4, 3], [4, 0, 3]])
    return V, T, 0.5


def duplicates_after_weld():
    """triangles on distinct indices that become equal (one rotated, one reversed) only through the weld"""
    V = _v([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 1, 0], [1, 0, 0], [0, 0, 0]])
    return V, _t([[0, 1, 2], [4, 5, 3], [6, 7, 8]]), 0.5


def collapsed_after_weld():
    """triangles with three distinct indices of which two or three coincide, next to one that was collapsed before"""
    V = _v([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 0], [1, 0, 0], [2, 2, 2], [2, 2, 2], [2, 2, 2]])
    return V, _t([[0, 1, 2], [0, 3, 2], [1, 4, 0], [5, 6, 7], [2, 2, 1], [3, 4, 2]]), 0.5


def unused_vertices():
    """vertex 4 is unused before the weld; 5, 6, 7 are used only by a collapsed triangle and 8 only by a duplicate, so they are
    unused only after the drops; 9 is unused but equal to the used vertex 0"""
    V = _v([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [5, 5, 5], [6, 6, 6], [6, 6, 6], [7, 7, 7], [0, 0, 1], [0, 0, 0]])
    return V, _t([[0, 1, 2], [5, 6, 7], [0, 1, 3], [1, 8, 0]]), 0.5


def flag_mesh():
    """one mesh for every flag combination: merged vertices, a collapsed triangle, duplicates, an opposite pair, unused vertices"""
    V = _v([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [0, 0, 0], [1, 0, 0], [3, 3, 3], [4, 4, 4], [4, 4, 4], [0, 1, 0]])
    T = _t([[0, 1, 2], [4, 5, 9], [1, 2, 0], [0, 2, 1], [7, 8, 3], [0, 1, 3], [5, 3, 4], [3, 1, 0]])
    return V, T, 0.5


def snap_negative():
    """snap = 0.5: coordinates either side of 0 and exact multiples of snap.  floor sends -0.25 to cell -1 and +0.25 to cell 0
    (truncation would merge them), -0.5 to -1 with -0.25 and -0.75 to -2; 0.5 starts cell 1"""
    xs = [-0.75, -0.5, -0.25, -0.0, 0.0, 0.25, 0.5, 0.75, 1.0, -1.0, -1.25]
    V = _v([[x, 0.1, 0.1] for x in xs] + [[0.1, x, 0.1] for x in xs] + [[0.1, 0.1, x] for x in xs])
    T = _t([[i, i + 1, i + 2] for i in range(0, 31)])
    return V, T, 0.5


def snap_cell_faces():
    """snap = 1: 0.999 and 1.001 are 0.002 apart in different cells and stay apart; 1.001 and 1.999 are 0.998 apart in one cell and
    merge - grid snapping, not a distance tolerance.  The same along y and z, and across a negative face"""
    V = _v([[0.999, 0.5, 0.5], [1.001, 0.5, 0.5], [1.999, 0.5, 0.5], [0.5, 0.999, 0.5], [0.5, 1.001, 0.5], [0.5, 1.999, 0.5],
            [0.5, 0.5, 0.999], [0.5, 0.5, 1.001], [0.5, 0.5, 1.999], [-0.001, 0.5, 0.5], [0.001, 0.5, 0.5], [-0.999, 0.5, 0.5]])
    return V, _t([[0, 1, 2], [3, 4, 5], [6, 7, 8], [9, 10, 11], [0, 3, 6], [1, 4, 7]]), 1.0


def sphere_soup():
    """the soup of the extracted sphere of tests/mesh_shells_cases.py (vertices restated by tests/iso_ref.py): every vertex of the
    mesh is repeated once per triangle that uses it"""
    V, T = S.extracted("sphere33")
    return np.ascontiguousarray(V[T.ravel()]), None, float(S.SPACING) / 8


CASES = {"empty": empty, "no_tris": no_tris, "one_triangle": one_triangle, "all_one_point": all_one_point, "signed_zero": signed_zero,
         "denormal_and_huge": denormal_and_huge, "differ_in_one_axis": differ_in_one_axis, "runs_across_blocks": runs_across_blocks,
         "cube_soup": cube_soup, "rotations": rotations, "duplicates_after_weld": duplicates_after_weld,
         "collapsed_after_weld": collapsed_after_weld, "unused_vertices": unused_vertices, "flag_mesh": flag_mesh,
         "snap_negative": snap_negative, "snap_cell_faces": snap_cell_faces, "sphere_soup": sphere_soup}
# the cases that run with every flag combination (each_flag_alone and no_flags among them); the others run with the default
# flags DROP_COLLAPSED | DROP_UNUSED and with all three
FLAG_CASES = ("flag_mesh", "rotations", "duplicates_after_weld", "collapsed_after_weld", "unused_vertices")
ALL = tuple(CASES)

_cases = {}


def case(name):
    if name not in _cases:
        _cases[name] = CASES[name]()
    return _cases[name]


def flag_sets(name):
    return tuple(range(8)) if name in FLAG_CASES else (5, 7)


def variants(name):
    """(snap, flags) of every run of the case"""
    return [(s, f) for s in (0.0, case(name)[2]) for f in flag_sets(name)]
