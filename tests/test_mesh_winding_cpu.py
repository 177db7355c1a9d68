"""The definition of the winding number (include/rho2sdf_hip.h, r2s_mesh_index_winding) checked without a GPU: the numpy restatement
of tests/mesh_winding_ref.py equals the analytic inside on the cases that have one, for all six rays, on lattices whose points project
onto every vertex, edge and edge-on face; the exact rational pair test finds no pair whose computed verdict differs from the exact
one on the named cases; and the per-point conditions are monotone along a lattice row, the property the row kernels rest on."""
import numpy as np
import pytest

import mesh_winding_cases as C
import mesh_winding_ref as R


@pytest.mark.parametrize("name", ["empty", "tetrahedron", "cube22", "octahedra", "two_cubes", "inward_cube", "collapsed_cube"])
def test_restatement_equals_the_analytic_winding(name):
    P = C.points(name)
    off = ~C.on_surface(name, P)
    want = C.truth(name, P)
    for ray in R.RAYS:
        wn, nc = C.expected(name, ray)
        assert np.array_equal(wn[off], want[off]), (name, ray, np.nonzero(wn[off] != want[off])[0][:5])
        assert (nc[~np.isfinite(P).all(axis=1)] == -1).all() and (wn[~np.isfinite(P).all(axis=1)] == 0).all()
        assert (nc[off] >= np.abs(wn[off])).all() and ((nc[off] - wn[off]) % 2 == 0).all()


def test_lattice_pair_counts():
    """the cube's half-integer and the octahedra's quarter-integer lattice: 1 470 and 53 910 (point, ray) pairs off the surface"""
    n_cube = int((~C.on_surface("cube22", C.lattice_points(C.lattice("cube22")))).sum())
    n_octa = int((~C.on_surface("octahedra", C.lattice_points(C.lattice("octahedra")))).sum())
    assert 6 * n_cube == 1470 and 6 * n_octa == 53910


def test_inside_rules():
    P = C.points("inward_cube")
    off = ~C.on_surface("inward_cube", P)
    box = C.in_box(P, 0, 2).astype(bool)
    for ray in R.RAYS:
        wn, nc = C.expected("inward_cube", ray)
        assert not R.inside(wn, nc, R.POSITIVE)[off].any()             # an inward cube is outside under POSITIVE,
        assert np.array_equal(R.inside(wn, nc, R.NONZERO)[off], box[off])   # inside under NONZERO
        assert np.array_equal(R.inside(wn, nc, R.ODD)[off], box[off])       # and under ODD
    P = C.points("reversed_cube")
    off = ~C.on_surface("reversed_cube", P)
    box = C.in_box(P, 0, 2).astype(bool)
    differs = 0
    for ray in R.RAYS:
        wn, nc = C.expected("reversed_cube", ray)
        assert np.array_equal(R.inside(wn, nc, R.ODD)[off], box[off]), ray    # ODD survives inconsistent winding;
        differs += int((R.inside(wn, nc, R.POSITIVE)[off] != box[off]).sum())   # the winding need not
    print(f"reversed_cube: POSITIVE differs from the truth at {differs} (point, ray) pairs")
    assert differs > 0, "the case reverses no triangle a ray meets (a mistake in this test)"
    wn, _ = C.expected("two_cubes", 2)
    P = C.points("two_cubes")
    assert (wn[((P > 1) & (P < 2)).all(axis=1)] == 2).all()


@pytest.mark.parametrize("name", C.ANALYTIC)
def test_exact_pair_test_agrees(name):
    V, T = C.case(name)
    P = C.points(name)
    examined = bad = 0
    for ray in R.RAYS:
        e, b = R.exact_disagreements(V, T, P, ray)
        examined, bad = examined + e, bad + b
    print(f"{name}: {examined} pairs examined exactly, {bad} disagreements")
    assert bad == 0


def test_exact_pair_test_on_a_random_soup_is_only_reported():
    """the documented limit, measured: float32 vertices in general position, points among them; nothing is asserted on the count"""
    rng = np.random.default_rng(11)
    V = rng.uniform(-1, 1, size=(90, 3)).astype(np.float32)
    T = np.arange(90, dtype=np.int32).reshape(-1, 3)
    P = np.concatenate([rng.uniform(-1, 1, size=(200, 3)), V[:40].astype(np.float64)])   # (also rays through vertices)
    total = [0, 0]
    for ray in R.RAYS:
        e, b = R.exact_disagreements(V, T, P, ray)
        total[0] += e
        total[1] += b
    print(f"random soup: {total[0]} pairs examined exactly, {total[1]} disagreements")
    assert total[0] > 0


def test_row_predicate_is_monotone():
    """along a row in the ray's axis, "the box reaches ahead, det != 0 and t > 0" switches at most once, from true to false for
    ray < 3 and from false to true for ray >= 3: every step of t is monotone in o[kz].  Seeded triangles and rows, also far away."""
    rng = np.random.default_rng(5)
    for trial in range(300):
        shift = np.zeros(3) if trial % 3 else np.array([1e3, -2e3, 5e2])
        h = (0.1, 0.0625, 1.0 / 3.0)[trial % 3]
        tri = (rng.uniform(-1, 1, size=(3, 3)) + shift).astype(np.float32)
        ray = trial % 6
        kx, ky, kz, _ = R.frame(ray)
        base = tri.astype(np.float64).mean(axis=0) + rng.normal(scale=0.2, size=3)
        base[kz] = tri[:, kz].min() - 1.5
        ok = R.predicate_along_row(tri[0], tri[1], tri[2], base, h, 65, ray)
        steps = np.diff(ok.astype(np.int8))
        assert np.count_nonzero(steps) <= 1 and ((steps <= 0).all() if ray < 3 else (steps >= 0).all()), (trial, ray, ok)
