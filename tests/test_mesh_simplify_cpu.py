"""The restatement of r2s_mesh_simplify (tests/mesh_simplify_ref.py) against itself and against analytic answers; no GPU.
simplify_ref(check=True) asserts its summation bound on every case it runs; the tolerances below are derived from that bound:
a Float64 sum is off by at most (n + K) 2^-53 T, the solve keeps directions with lambda >= 1e-3 lambda_max and so amplifies that
by at most 1e3, and the result is rounded once to float32."""
import os
import re

import numpy as np
import pytest

import mesh_simplify_cases as C
import mesh_simplify_ref as R
from conftest import ROOT

RULES = (R.MEAN, R.QUADRIC)
CASES = dict(C.all_cases())
NAMES = list(CASES)
_refs = {}


def ref(name, rule):
    if (name, rule) not in _refs:
        _refs[name, rule] = R.simplify_ref(*CASES[name], rule, check=True)
    return _refs[name, rule]


def position_tol(r, v, cell, extent):
    """the Float64 stage, (n + K) 2^-53 amplified by 1e3 on a length of `extent`, plus one float32 ulp of the largest coordinate"""
    return 1e3 * (r["items_max"] + R.K) * 2.0 ** -53 * extent + float(np.spacing(np.float32(np.abs(v).max())))


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("name", NAMES)
def test_counts_are_consistent(name, rule):
    v, t, cell = CASES[name]
    r = ref(name, rule)
    tot = r["totals"]
    assert tot[0] == len(r["verts"]) == len(r["members"]) and tot[1] == len(r["tris"]) == (r["tri_map"] >= 0).sum()
    assert r["members"].sum() == (r["vert_map"] >= 0).sum() and tot[2] + tot[0] + tot[6] == len(v)
    if len(r["tris"]):
        assert r["tris"].min() >= 0 and r["tris"].max() < tot[0]
        a, b, c = r["tris"].T
        assert ((a != b) & (b != c) & (a != c)).all()
    first = [int(np.nonzero(r["vert_map"] == c)[0][0]) for c in range(tot[0])]
    assert first == sorted(first)                        # first-occurrence order of the first member


def test_named_cases():
    assert ref("empty", R.QUADRIC)["totals"].tolist() == [0] * 8
    assert ref("one_triangle_one_cell", R.QUADRIC)["totals"].tolist() == [0, 0, 3, 1, 0, 0, 0, 0]
    assert ref("one_triangle_three_cells", R.QUADRIC)["totals"][:7].tolist() == [3, 1, 0, 0, 0, 0, 0]
    d = ref("duplicate_pair", R.QUADRIC)
    assert d["totals"][:7].tolist() == [3, 1, 1, 0, 1, 0, 0] and d["tri_map"].tolist() == [0, -1]
    assert R.simplify_ref(*CASES["duplicate_pair"], R.QUADRIC, drop_duplicates=False)["totals"][:7].tolist() == [3, 2, 1, 0, 1, 0, 0]
    o = ref("opposite_pair", R.QUADRIC)
    assert o["totals"][:7].tolist() == [3, 2, 1, 0, 0, 1, 0]
    n = ref("non_members", R.QUADRIC)
    assert n["totals"][:7].tolist() == [3, 1, 0, 1, 0, 0, 2] and n["vert_map"].tolist() == [0, 1, 2, -1, -1]
    z = ref("zero_area", R.QUADRIC)
    assert (z["solved"] == 0).all() and np.array_equal(z["verts"], ref("zero_area", R.MEAN)["verts"])
    two = ref("two_corners_one_class", R.QUADRIC)
    assert two["members"].tolist() == [2, 1, 1, 1] and two["totals"][3] == 1
    b = ref("cell_boundaries", R.MEAN)
    assert b["vert_map"][0] == b["vert_map"][4] and b["totals"][0] == 7    # -0.0 and +0.0 share the cell 0; a vertex ON k * cell is in cell k
    for n_members in (255, 256, 257, 5000):
        assert ref(f"fan_{n_members}", R.QUADRIC)["members"][0] == n_members


@pytest.mark.parametrize("name", [n for n in NAMES if n.endswith("+permuted")])
def test_permutation_follows(name):
    """the partition and every integer follow a permutation of the input up to the renumbering"""
    for rule in RULES:
        a, b = ref(name.split("+")[0], rule), ref(name, rule)
        assert np.array_equal(a["totals"][:7], b["totals"][:7])
        assert sorted(a["members"].tolist()) == sorted(b["members"].tolist())
        back = np.random.default_rng(7).permutation(len(CASES[name][0]))   # permuted vertex j is original vertex back[j] (C.permuted)
        assert np.array_equal(CASES[name][0], CASES[name.split("+")[0]][0][back])
        pa = sorted(tuple(sorted(np.nonzero(a["vert_map"] == c)[0])) for c in range(a["totals"][0]))
        pb = sorted(tuple(sorted(back[np.nonzero(b["vert_map"] == c)[0]])) for c in range(b["totals"][0]))
        assert pa == pb


def _cube_axes(v):
    lo, hi = v.min(0), v.max(0)
    return (v == lo) | (v == hi)


def test_cube_quadric_keeps_corners_edges_faces():
    v, t, cell = CASES["cube"]
    r = ref("cube", R.QUADRIC)
    tol = position_tol(r, v, cell, 1.0)
    on = _cube_axes(v)
    kinds = {1: 0, 2: 0, 3: 0}
    for c in range(len(r["verts"])):
        mem = np.nonzero(r["vert_map"] == c)[0]
        pinned = [k for k in range(3) if on[mem, k].any()]
        kinds[len(pinned)] += 1
        for k in pinned:                                 # a corner class: all three, an edge class: two, a face class: one
            assert abs(float(r["verts"][c, k]) - float(v[mem[on[mem, k]][0], k])) <= tol, (c, k)
        assert r["solved"][c] & 3 == len(pinned)
    assert kinds[3] == 8 and kinds[2] > 0 and kinds[1] > 0


def test_cube_mean_rounds_the_cube_off():
    """the mean of a corner class that holds edge and face vertices lies strictly inside the cube: with the coordinates 0.55 and
    0.8 per axis in the cell, the seven surface vertices of the class average to 0.8 - 0.25 * 3 / 7 on every axis"""
    v, t, cell = CASES["cube"]
    r = ref("cube", R.MEAN)
    on = _cube_axes(v)
    hi = v.max(0)
    c = int(r["vert_map"][np.nonzero((v == hi).all(1))[0][0]])
    assert r["members"][c] == 7
    want = float(hi[0]) - 0.25 * 3 / 7
    assert np.abs(r["verts"][c].astype(np.float64) - want).max() <= 1e-6
    gap = max(abs(float(r["verts"][k, a]) - float(v[m, a])) for k in range(len(r["verts"]))
              for m in np.nonzero(r["vert_map"] == k)[0] for a in range(3) if on[m, a])
    assert gap >= 0.25 * 3 / 7 - 1e-6


@pytest.mark.parametrize("rule", RULES)
def test_plane_patch_stays_in_the_plane(rule):
    v, t, cell = CASES["plane_patch"]
    r = ref("plane_patch", rule)
    assert len(r["verts"]) > 4
    assert np.abs(r["verts"][:, 2].astype(np.float64) - float(v[0, 2])).max() <= position_tol(r, v, cell, 1.0)
    if rule == R.QUADRIC:
        assert (r["solved"] & 3 == 1).all()


def test_crease_has_rank_two_classes():
    v, t, cell = CASES["crease"]
    r = ref("crease", R.QUADRIC)
    tol = position_tol(r, v, cell, 1.0)
    two = (r["solved"] & 3) == 2
    assert two.any() and ((r["solved"] & 3)[~two] == 1).all()
    x = r["verts"].astype(np.float64)
    assert np.abs(x[two, 1] - float(np.float32(0.5))).max() <= tol and np.abs(x[two, 2] - float(np.float32(0.1))).max() <= tol


def _slack(E, c, point, cell, items_max):
    """|E(p + e) - E(p)| <= 2 sqrt(E(p) tr(S)) |e| + tr(S) |e|^2 for the rounding e the definition allows: one float32 ulp per
    axis plus the Float64 solve error 1e3 (n + K) 2^-53 cell"""
    e = 3 ** 0.5 * (float(np.spacing(np.float32(np.abs(point).max()))) + 1e3 * (items_max + R.K) * 2.0 ** -53 * cell)
    tr = float(E.trace(c))
    return 2.0 * (float(E(c, point)) * tr) ** 0.5 * e + tr * e * e


@pytest.mark.parametrize("name", NAMES)
def test_quadric_is_no_worse_than_the_mean(name):
    """E(x) <= E(m) for every class, compared in Fraction from the float32 outputs"""
    v, t, cell = CASES[name]
    q, m = ref(name, R.QUADRIC), ref(name, R.MEAN)
    if not len(q["verts"]):
        return
    E = R.exact_quadric(v, t, q["vert_map"])
    for c in range(len(q["verts"])):
        gain = float(E(c, q["verts"][c]) - E(c, m["verts"][c]))
        assert gain <= _slack(E, c, q["verts"][c], cell, q["items_max"]) + _slack(E, c, m["verts"][c], cell, q["items_max"]), c


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("name", NAMES)
def test_representatives_lie_in_their_cells(name, rule):
    v, t, cell = CASES[name]
    r = ref(name, rule)
    x = r["verts"].astype(np.float64)
    lo, hi = r["cells"] * cell, (r["cells"] + 1.0) * cell
    ulp = np.spacing(np.maximum(np.abs(lo), np.abs(hi)).astype(np.float32)).astype(np.float64)   # of the cell's larger face coordinate
    assert (x >= lo - ulp).all() and (x <= hi + ulp).all()
    assert np.array_equal(r["cells"], R.cells_of(v, cell)[[int(np.nonzero(r["vert_map"] == c)[0][0]) for c in range(len(x))]].reshape(-1, 3))


SMALL = [n for n in NAMES if len(CASES[n][1]) <= 600 and "fan" not in n]


@pytest.mark.parametrize("name", SMALL)
def test_deviation_bound(name):
    """every vertex and edge midpoint of every surviving input triangle is within sqrt(3) * cell of the simplified surface: each
    vertex moves inside its cell, and a barycentric mix of the moves is no longer than the longest of them"""
    v, t, cell = CASES[name]
    r = ref(name, R.QUADRIC)
    if not len(r["tris"]):
        return
    kept = t[r["tri_map"] >= 0]
    V = v.astype(np.float64)
    pts = np.concatenate([V[kept].reshape(-1, 3), 0.5 * (V[kept] + V[kept][:, [1, 2, 0]]).reshape(-1, 3)])
    pts = np.unique(pts, axis=0)[::max(1, len(pts) // 400)]
    assert R.distance_to_mesh(pts, r["verts"], r["tris"]).max() <= 3 ** 0.5 * cell * (1 + 1e-6)


@pytest.mark.parametrize("name", NAMES)
def test_share_of_classes_without_a_margin(name):
    """at most 1 % on every named case.  The recorded extractor meshes cannot meet that at any cell (a sphere sampled finer than
    its curvature has eigenvalue ratios of about (cell / radius)^2 spread across the 1e-3 threshold; box faces put optima ON cell
    faces), so there every class without a margin must list the result of each decision it could take, and an implementation
    is compared with those: no class is left uncompared."""
    r = ref(name, R.QUADRIC)
    und = r["undecidable"]
    if name in C.recorded():
        assert all(len(r["candidates"][c]) >= 2 for c in np.nonzero(und)[0])
    else:
        assert und.sum() <= 0.01 * len(und), int(und.sum())
    assert all(len(r["candidates"][c]) == 1 for c in np.nonzero(~und)[0])
    for c in range(len(und)):                            # the definition's own result comes first
        assert r["candidates"][c][0][0] == r["solved"][c] and np.array_equal(r["candidates"][c][0][1], r["verts"][c])


def test_python_exports_and_bindings(pkg):
    for name in ("MeshSimplify", "mesh_simplify", "mesh_simplify_dev"):
        assert name in pkg.__all__ and hasattr(pkg, name)
    names = [s[0] for s in pkg._lib.SYMBOLS]
    for s in ("r2s_mesh_simplify", "r2s_mesh_simplify_dev", "r2s_last_mesh_simplify"):
        assert names.count(s) == 1
    hdr = open(os.path.join(ROOT, "include", "rho2sdf_hip.h")).read()
    assert re.search(r"#define R2S_SIMPLIFY_MEAN 0\b", hdr) and re.search(r"#define R2S_SIMPLIFY_QUADRIC 1\b", hdr)
    assert (pkg._lib.SIMPLIFY_MEAN, pkg._lib.SIMPLIFY_QUADRIC) == (0, 1)
    julia = open(os.path.join(ROOT, "rho2sdf.jl_amd", "julia", "Rho2sdfHIP.jl")).read()
    for s in (":r2s_mesh_simplify,", ":r2s_mesh_simplify_dev,", ":r2s_last_mesh_simplify,"):
        assert s in julia, s
    with pytest.raises(pkg._lib.R2SError):
        pkg.mesh_simplify(np.zeros((3, 3), np.float32), np.array([[0, 1, 2]], np.int32), 1.0, "best")
