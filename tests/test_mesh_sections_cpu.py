"""No GPU: the yardstick of tests/test_mesh_sections_gpu.py and the CPU side of the binding (include/rho2sdf_hip.h,
r2s_mesh_sections).  The restatement (mesh_sections_ref64) is held to its own bound against exact `fractions` arithmetic on the
hand-made cases, under three summation orders; known answers; the header declares and the library exports the three entry
points; the refusals that need no device return their codes; MeshSections' derived values on hand-made input."""
import ctypes
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import mesh_sections_cases as C
import mesh_sections_ref64 as M

ARG, NO_DEVICE, UNSUPPORTED = -1, -2, -4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = tuple(n for n in C.HAND if n != "band20000")          # (20 000 segments in rational arithmetic take too long)
_ref = {}


def _restated(name):
    if name not in _ref:
        _ref[name] = M.sections(*C.case(name))
    return _ref[name]


def _sqrt(q, bits=200):
    """the square root of a Fraction to 2^-bits of its size"""
    return Fraction(math.isqrt((q.numerator << (2 * bits)) // q.denominator), 1 << bits) if q > 0 else Fraction(0)


def _exact_terms(pts, r, normal):
    """the header's seven terms of every segment from the double points, in exact rational arithmetic (the square root to
    200 bits)"""
    n = [Fraction(float(x)) for x in normal]
    rr = [Fraction(float(x)) for x in r]
    out = []
    for fr, to in pts:
        A = [Fraction(float(x)) - q for x, q in zip(fr, rr)]
        B = [Fraction(float(x)) - q for x, q in zip(to, rr)]
        D = [b - a for a, b in zip(A, B)]
        Cv = [A[1] * B[2] - A[2] * B[1], A[2] * B[0] - A[0] * B[2], A[0] * B[1] - A[1] * B[0]]
        w = sum(x * y for x, y in zip(n, Cv))
        out.append([_sqrt(sum(d * d for d in D))] + Cv + [w * (a + b) for a, b in zip(A, B)])
    return out


def _pairwise(x):
    x = np.array(x)
    while len(x) > 1:
        if len(x) % 2:
            x = np.concatenate([x, np.zeros((1, x.shape[1]))])
        x = x[0::2] + x[1::2]
    return x[0]


@pytest.mark.parametrize("name", SMALL)
def test_restatement_within_its_bound_against_exact_fractions(name):
    r = _restated(name)
    exact = _exact_terms(r["seg_points"], r["ref_point"], r["normal"])
    start, worst = r["contour_start"], 0.0
    for c in range(len(r["counts"])):
        lo, hi = int(start[c]), int(start[c + 1])
        want = [sum(col) for col in zip(*exact[lo:hi])]
        x = r["terms"][lo:hi]
        orders = {"sequential": np.cumsum(x, axis=0)[-1], "reversed": np.cumsum(x[::-1], axis=0)[-1], "pairwise": _pairwise(x)}
        assert (orders["sequential"] == r["sums"][c]).all()
        for label, got in orders.items():
            err = np.array([float(abs(Fraction(float(g)) - w)) for g, w in zip(got, want)])
            b = r["bound"][c]
            assert (err <= b).all(), (name, c, label, err.tolist(), b.tolist())
            worst = max(worst, float((err[b > 0] / b[b > 0]).max()) if (b > 0).any() else 0.0)
    print(f"SECTIONS yardstick {name}: {r['totals'][1]} segments, {r['totals'][0]} contours, largest fraction of the bound {worst:.3f}")


def _area(r):
    n = r["normal"]
    return 0.5 * (r["sums"][:, 1:4] @ n) / np.sqrt(n @ n)


def test_corner_tetrahedron_areas_are_exact():
    """L = 60, normal z, level c: the section is the right triangle with legs 60 - c.  Where (c / 60) * 60 == c in double (every
    integer c but 31) the points are integers, every term is an integer below 2^53 and the area is (60 - c)^2 / 2 exactly;
    elsewhere within the bound"""
    r = _restated("tet_integer_levels")
    c = r["levels"]
    assert r["totals"].tolist() == [59, 177, 0, 177, 0, 0, 0, 59] and (r["counts"][:, 2] == 3).all()
    exact = (c / 60.0) * 60.0 == c
    assert exact.sum() >= 55
    area = _area(r)
    assert (area[exact] == ((60.0 - c) ** 2 / 2)[exact]).all()
    assert (np.abs(area - (60.0 - c) ** 2 / 2) <= 0.5 * r["bound"][:, 3]).all()


def test_cube_with_a_level_on_a_face():
    assert _restated("cube_bottom")["totals"].tolist() == [0] * 8          # h >= c everywhere: nothing is below
    r = _restated("cube_top")
    V = C.case("cube_top")[0].astype(np.float64)
    assert r["totals"].tolist() == [1, 8, 0, 8, 0, 0, 0, 1] and r["closed"].all()
    assert _area(r).tolist() == [2.25] and r["sums"][0, 0] == 6.0
    top = {tuple(p) for p in V[V[:, 2] == 1.5]}
    assert {tuple(p) for p in r["seg_points"].reshape(-1, 3)} == top      # bit-equal to the four vertices of the face
    # counter-clockwise seen from +z: the corners in the order of the walk, without the zero-length segments
    walk = [tuple(p) for p, q in r["seg_points"] if tuple(p) != tuple(q)]
    assert walk == [(0.0, 0.0, 1.5), (1.5, 0.0, 1.5), (1.5, 1.5, 1.5), (0.0, 1.5, 1.5)]


def test_expected_shapes_of_the_hand_made_cases():
    want = {"empty": [0] * 8, "no_levels": [0] * 8, "levels_outside": [0] * 8, "all_collapsed": [0, 0, 4, 0, 0, 0, 0, 0],
            "one_triangle": [2, 2, 0, 4, 4, 0, 0, 0], "three_on_edge": [2, 6, 0, 8, 6, 0, 2, 0],
            "triangle_twice": [1, 2, 0, 2, 0, 2, 0, 0], "cube_with_void": [4, 32, 0, 32, 0, 0, 0, 4],
            "stacked_cubes": [4, 24, 0, 24, 0, 0, 0, 4], "tet_vertex_levels_z": [1, 3, 0, 3, 0, 0, 0, 1],
            "tet_vertex_levels_111": [1, 3, 0, 3, 0, 0, 0, 1], "band20000": [1, 20000, 0, 20000, 0, 0, 0, 1]}
    for name, tot in want.items():
        assert _restated(name)["totals"].tolist() == tot, name
    assert _restated("cube_one_reversed")["totals"][5] == 4
    r = _restated("cube_with_void")
    assert r["counts"][:, 0].tolist() == [0, 1, 1, 2] and _area(r).tolist() == [4.0, 4.0, -1.0, 4.0]
    r = _restated("stacked_cubes")          # contours of neighbouring levels with bit-equal points stay apart
    s = r["contour_start"]
    for a, b in ((0, 1), (2, 3)):
        pa, pb = r["seg_points"][s[a]:s[a + 1]].reshape(-1, 6), r["seg_points"][s[b]:s[b + 1]].reshape(-1, 6)
        assert {tuple(x) for x in pa} == {tuple(x) for x in pb}
    r = _restated("tet_1000_levels")
    assert r["totals"][0] == 1000 and r["closed"].all() and set(r["counts"][:, 2].tolist()) == {3, 4}
    for name in ("tet_vertex_levels_z", "tet_vertex_levels_111", "torus_saddle", "torus_123", "cones"):
        assert _restated(name)["closed"].all(), name
    r = _restated("torus_123")
    assert (np.bincount(r["counts"][:, 0], minlength=6)[1:5] == 2).all()   # through the hole: two loops per level
    r = _restated("cones")
    assert sorted(r["counts"][:, 2].tolist()) == sorted(2 * list(C.LOOP_SIZES))


def test_header_declares_and_library_exports_the_symbols(pkg):
    names = ("r2s_mesh_sections", "r2s_last_mesh_sections", "r2s_mesh_sections_dev")
    with open(os.path.join(ROOT, "include", "rho2sdf_hip.h")) as f:
        header = f.read()
    lib = pkg._lib.lib()
    for name in names:
        assert re.search(r"^int " + name + r"\(", header, re.M), name
        assert getattr(lib, name) is not None
    assert {"mesh_sections", "mesh_sections_dev", "MeshSections"} <= set(pkg.__all__)


def _call(pkg, V, T, normal=C.Z, levels=(0.5,), nl=None, outs=True):
    L = pkg._lib
    V, T = np.ascontiguousarray(V, np.float32), np.ascontiguousarray(T, np.int32)
    nrm = None if normal is None else np.asarray(normal, np.float64)
    lev = None if levels is None else np.asarray(levels, np.float64)
    nc, ns, ref, tot = ctypes.c_int64(-7), ctypes.c_int64(-7), np.full(3, -7.0), np.full(8, -7, np.int64)
    rc = L.lib().r2s_mesh_sections(V.ctypes.data_as(L.c_float_p), len(V), T.ctypes.data_as(L.c_int32_p), len(T),
                                   None if nrm is None else nrm.ctypes.data_as(L.c_double_p),
                                   None if lev is None or not lev.size else lev.ctypes.data_as(L.c_double_p),
                                   (0 if lev is None else len(lev)) if nl is None else nl, -1, ctypes.byref(nc) if outs else None,
                                   ctypes.byref(ns), ref.ctypes.data_as(L.c_double_p), tot.ctypes.data_as(L.c_int64_p))
    return rc, nc.value == -7 and ns.value == -7 and (ref == -7.0).all() and (tot == -7).all()


def test_refusals_need_no_device(pkg):
    V, T = C.S.cube((0, 0, 0), 1.0)
    for normal in ((0.0, 0.0, 0.0), (np.nan, 0.0, 1.0), (0.0, np.inf, 1.0), (0.0, 0.0, 2.0 ** 501), None):
        assert _call(pkg, V, T, normal=normal) == (ARG, True), normal
    for levels in ((0.5, 0.5), (0.5, 0.25), (0.0, np.nan), (np.inf,), (-np.inf, 0.0)):
        assert _call(pkg, V, T, levels=levels) == (ARG, True), levels
    assert _call(pkg, V, T, levels=None, nl=3) == (ARG, True) and _call(pkg, V, T, nl=-1) == (ARG, True)
    assert _call(pkg, V, T, nl=2 ** 30 + 1) == (UNSUPPORTED, True)
    assert _call(pkg, V, T, outs=False) == (ARG, True)
    T2 = T.copy()
    T2[7, 1] = 8
    assert _call(pkg, V, T2) == (ARG, True)
    lib = pkg._lib.lib()
    n = ctypes.c_int64()
    assert lib.r2s_last_mesh_sections(None, None, None, 4, None, None, 0, ctypes.byref(n), ctypes.byref(n)) == ARG
    assert lib.r2s_last_mesh_sections(None, None, None, 0, None, None, 4, ctypes.byref(n), ctypes.byref(n)) == ARG
    assert lib.r2s_last_mesh_sections(None, None, None, 0, None, None, 0, None, None) == ARG
    assert lib.r2s_mesh_sections_dev(None, 0, None, 0, None, None, 0, None, None, None, 0, None, None, 0, None, None, None, None, None) == ARG
    with pytest.raises(pkg._lib.R2SError, match="info"):
        pkg.rho2sdf("t", np.zeros((8, 3)), np.arange(1, 9)[None, :], np.ones(1), sections=(C.Z, [0.0]))


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present")
def test_no_cpu_fallback(pkg):
    V, T = C.S.cube((0, 0, 0), 1.0)
    assert _call(pkg, V, T) == (NO_DEVICE, True)
    with pytest.raises(pkg._lib.R2SError, match="no HIP device|CPU fallback"):
        pkg.mesh_sections(V, T, C.Z, [0.5])


def test_derived_values_on_hand_made_input(pkg):
    V, T, normal, levels = C.case("cube_with_void")
    r = _restated("cube_with_void")
    s = pkg.MeshSections(normal, levels, r["contour_start"], r["counts"], r["sums"], r["ref_point"], r["totals"], r["seg_tri"],
                         r["seg_points"])
    assert s.n_contours == 4 and s.closed.all() and s.is_hole.tolist() == [False, False, True, False]
    assert s.area.tolist() == [4.0, 4.0, -1.0, 4.0] and s.length.tolist() == [8.0, 8.0, 4.0, 8.0]
    assert s.level_n_contours.tolist() == [1, 2, 1] and s.level_area.tolist() == [4.0, 3.0, 4.0]
    assert s.level_perimeter.tolist() == [8.0, 12.0, 8.0]
    assert np.allclose(s.centroid, [[1, 1, 0.25], [1, 1, 1], [1, 1, 1], [1, 1, 1.75]], atol=1e-14)
    assert np.allclose(s.level_centroid, [[1, 1, 0.25], [1, 1, 1], [1, 1, 1.75]], atol=1e-14)
    loops = s.loops(1)
    assert len(loops) == 2 and loops[0].shape == (8, 3) and (loops[0][:, 2] == 1.0).all() and s.loops(0)[0].shape == (8, 3)
    o = _restated("one_triangle")
    V1, T1, n1, l1 = C.case("one_triangle")
    o = pkg.MeshSections(n1, l1, o["contour_start"], o["counts"], o["sums"], o["ref_point"], o["totals"], o["seg_tri"], o["seg_points"])
    assert not o.closed.any() and np.isnan(o.centroid).all() and o.loops(0) == [] and (o.level_area == 0).all()
