"""The mesh sections on the GPU (r2s_mesh_sections, r2s_mesh_sections_dev, rho2sdf(sections=...)) against the restatement of
tests/mesh_sections_ref64.py on every case of tests/mesh_sections_cases.py: seg_tri, contour_start, every integer record, the
totals, the reference point and EVERY POINT bit for bit, every Float64 sum within

    bound(c) = (n_segs(c) + K) * 2^-53 * T(c)

(K and T as in the restatement; tests/test_mesh_sections_cpu.py holds the restatement itself to that bound against exact
rational arithmetic).  Each case prints the largest fraction of the bound used as a "SECTIONS ..." line.

What the cases reach:
    empty, no_levels, levels_outside, all_collapsed, cube_bottom    zero segments
    one_triangle, noise24_open, gyroid17                            open ends; contours that are not closed keep id order
    three_on_edge                                                   a branch node
    triangle_twice, cube_one_reversed                               flipped nodes
    cube_with_void                                                  a hole (negative area); two contours on one level
    stacked_cubes                                                   contours of different levels with bit-equal points
    tet_1000_levels                                                 many segments per triangle, loops of 3 and 4 segments
    tet_vertex_levels_*, torus_saddle, cube_top                     the >= rule: vertices exactly on a level, all closed
    band20000                                                       one loop of 20 000 segments: more than 64 block partials,
                                                                    15 rounds of pointer jumping
    cones                                                           loops of 255, 256, 257 and 2^k +- 1 segments, shuffled
    torus_123                                                       two loops per level, unnormalised general normal
    sphere33, gyroid17, noise24_*                                   extracted meshes with vertices exactly on levels"""
import ctypes

import numpy as np
import pytest

import mesh_sections_cases as C
import mesh_sections_ref64 as M
from conftest import load_fixture

pytestmark = pytest.mark.gpu

_ref = {}


def _restated(name):
    """the restatement of a case, computed once and left unchanged"""
    if name not in _ref:
        _ref[name] = M.sections(*C.case(name))
    return _ref[name]


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _host(s):
    """a result of mesh_sections_dev with its device tables brought to the host"""
    if hasattr(s.seg_tri, "cpu"):
        s.seg_tri, s.seg_points = s.seg_tri.cpu().numpy(), s.seg_points.cpu().numpy()
    return s


def _same(a, b):
    """two results bit for bit"""
    return (np.array_equal(a.contour_start, b.contour_start) and np.array_equal(a.counts, b.counts)
            and np.array_equal(_bits(a.sums), _bits(b.sums)) and np.array_equal(a.totals, b.totals)
            and np.array_equal(_bits(a.ref_point), _bits(b.ref_point)) and np.array_equal(a.seg_tri, b.seg_tri)
            and np.array_equal(_bits(a.seg_points), _bits(b.seg_points)))


def _check(label, s, r):
    assert np.array_equal(s.totals, r["totals"]), (label, s.totals.tolist(), r["totals"].tolist())
    assert np.array_equal(s.counts, r["counts"]), label
    assert np.array_equal(s.contour_start, r["contour_start"]), label
    assert np.array_equal(s.seg_tri, r["seg_tri"]), label
    assert np.array_equal(_bits(s.ref_point), _bits(r["ref_point"])), label
    assert np.array_equal(_bits(s.seg_points), _bits(r["seg_points"])), label
    err, b = np.abs(s.sums - r["sums"]), r["bound"]
    frac = float((err[b > 0] / b[b > 0]).max()) if (b > 0).any() else 0.0
    print(f"SECTIONS {label}: {s.totals[1]} segments, {s.n_contours} contours, {s.totals[7]} closed, "
          f"largest fraction of the bound {frac:.4f}")
    assert (err <= b).all(), (label, frac)


def _dev(pkg, case, stream=None, **capacities):
    import torch
    V, T, normal, levels = case
    v, t = torch.from_numpy(np.ascontiguousarray(V)).cuda(), torch.from_numpy(np.ascontiguousarray(T)).cuda()
    return _host(pkg.mesh_sections_dev(v, t, normal, levels, stream, **capacities))


@pytest.mark.parametrize("name", C.ALL)
def test_equal_to_the_restatement(pkg, name):
    _check(name, pkg.mesh_sections(*C.case(name)), _restated(name))


def test_what_the_cases_must_show(pkg):
    sec = {name: pkg.mesh_sections(*C.case(name)) for name in C.ALL}
    for name in ("empty", "no_levels", "levels_outside", "cube_bottom"):
        assert sec[name].totals.tolist() == [0] * 8 and sec[name].n_contours == 0 and len(sec[name].seg_tri) == 0, name
    assert sec["all_collapsed"].totals.tolist() == [0, 0, 4, 0, 0, 0, 0, 0]
    s = sec["one_triangle"]
    assert s.n_open.tolist() == [2, 2] and not s.closed.any()
    assert sec["three_on_edge"].n_branch.tolist() == [1, 1]
    assert sec["triangle_twice"].n_flipped.tolist() == [2] and sec["cube_one_reversed"].totals[5] == 4
    s = sec["cube_with_void"]
    assert s.level.tolist() == [0, 1, 1, 2] and s.area.tolist() == [4.0, 4.0, -1.0, 4.0] and s.is_hole.tolist() == [False, False, True, False]
    assert s.level_area.tolist() == [4.0, 3.0, 4.0]
    s = sec["cube_top"]          # a level exactly on the top face: one closed square, its points the face's vertices
    V = C.case("cube_top")[0].astype(np.float64)
    assert s.closed.tolist() == [True] and s.area.tolist() == [2.25]
    assert {tuple(p) for p in s.seg_points.reshape(-1, 3)} == {tuple(p) for p in V[V[:, 2] == 1.5]}
    s = sec["stacked_cubes"]
    assert s.n_contours == 4 and s.closed.all() and s.level.tolist() == [0, 1, 2, 3]
    s = sec["tet_integer_levels"]          # (the exact levels are those of tests/test_mesh_sections_cpu.py)
    c = s.levels
    ok = (c / 60.0) * 60.0 == c
    assert ok.sum() >= 55 and (s.area[ok] == ((60.0 - c) ** 2 / 2)[ok]).all()
    s = sec["tet_1000_levels"]
    assert s.n_contours == 1000 and s.closed.all() and set(s.n_segs.tolist()) == {3, 4}
    for name in ("tet_vertex_levels_z", "tet_vertex_levels_111", "torus_saddle", "torus_123", "cones", "sphere33", "noise24_closed"):
        assert sec[name].closed.all() and sec[name].n_contours > 0, name
    assert (sec["torus_123"].level_n_contours[1:5] == 2).all()
    s = sec["band20000"]
    assert s.n_segs.tolist() == [20000] and s.closed[0] and s.area[0] > 0 and len(s.loops(0)[0]) == 20000
    assert sorted(sec["cones"].n_segs.tolist()) == sorted(2 * list(C.LOOP_SIZES))
    assert sec["gyroid17"].n_open.sum() > 0 and sec["noise24_open"].n_open.sum() > 0
    s = sec["sphere33"]          # every second level lies exactly on a lattice plane: vertices on levels
    assert (s.area > 0).all() and (s.level_n_contours <= 1).all()


@pytest.mark.parametrize("name", ["noise24_open", "band20000", "cones", "tet_1000_levels"])
def test_reproducible_and_both_variants_bit_for_bit(pkg, name):
    case = C.case(name)
    a, b = pkg.mesh_sections(*case), pkg.mesh_sections(*case)
    assert _same(a, b)
    assert _same(a, _dev(pkg, case)) and _same(a, _dev(pkg, case, contour_capacity=a.n_contours + 5, segment_capacity=a.n_segments + 3))
    pkg._lib.lib().r2s_release_cache()                      # fresh work buffers
    assert _same(a, pkg.mesh_sections(*case))


def test_dev_on_a_non_default_stream_with_inputs_produced_on_it(pkg):
    import torch
    V, T, normal, levels = C.case("noise24_closed")
    want = pkg.mesh_sections(V, T, normal, levels)
    hv, ht = torch.from_numpy(V).pin_memory(), torch.from_numpy(T).pin_memory()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        v, t = torch.zeros(V.shape, dtype=torch.float32, device="cuda"), torch.zeros(T.shape, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(st):          # the copies that fill the inputs are queued on the stream and not waited for
        v.copy_(hv, non_blocking=True)
        t.copy_(ht, non_blocking=True)
        got = _host(pkg.mesh_sections_dev(v, t, normal, levels, st))
    assert _same(want, got)


def test_dev_short_capacity_leaves_the_tables_untouched(pkg):
    import torch
    L = pkg._lib
    V, T, normal, levels = C.case("cube_with_void")
    v, t = torch.from_numpy(V).cuda(), torch.from_numpy(T).cuda()
    start = torch.full((5,), -7, dtype=torch.int64, device="cuda")
    counts = torch.full((4, 8), -7, dtype=torch.int64, device="cuda")
    sums = torch.full((4, 7), -7.0, dtype=torch.float64, device="cuda")
    seg_tri = torch.full((32,), -7, dtype=torch.int32, device="cuda")
    pts = torch.full((32, 2, 3), -7.0, dtype=torch.float64, device="cuda")
    nc, ns, ref, tot = ctypes.c_int64(), ctypes.c_int64(), np.zeros(3), np.zeros(8, np.int64)
    vp = ctypes.c_void_p
    head = (vp(v.data_ptr()), len(V), vp(t.data_ptr()), len(T), normal.ctypes.data_as(L.c_double_p), levels.ctypes.data_as(L.c_double_p), 3)
    tail = (ctypes.byref(nc), ctypes.byref(ns), ref.ctypes.data_as(L.c_double_p), tot.ctypes.data_as(L.c_int64_p), None)

    def call(ccap, scap):
        L.check(L.lib().r2s_mesh_sections_dev(*head, vp(start.data_ptr()), vp(counts.data_ptr()), vp(sums.data_ptr()), ccap,
                                              vp(seg_tri.data_ptr()), vp(pts.data_ptr()), scap, *tail))

    for ccap, scap in ((0, 0), (3, 32), (4, 31)):
        call(ccap, scap)
        assert nc.value == 4 and ns.value == 32 and tot.tolist() == [4, 32, 0, 32, 0, 0, 0, 4] and (ref == 1.0).all()
        assert (start == -7).all() and (counts == -7).all() and (sums == -7.0).all() and (seg_tri == -7).all() and (pts == -7.0).all()
    call(4, 32)
    assert start.cpu().tolist() == [0, 8, 16, 24, 32] and counts.cpu().numpy()[:, 2].tolist() == [8] * 4
    assert (0.5 * sums.cpu().numpy()[:, 3]).tolist() == [4.0, 4.0, -1.0, 4.0] and (seg_tri >= 0).all()


@pytest.mark.parametrize("name", ["noise24_open", "band20000", "cones", "torus_123"])
def test_permutation_of_the_triangles(pkg, name):
    case = C.case(name)
    pcase, perm = C.permuted(case, 33)
    a, p = pkg.mesh_sections(*case), pkg.mesh_sections(*pcase)
    r = _restated(name)
    assert np.array_equal(a.totals, p.totals) and np.array_equal(a.level_n_contours, p.level_n_contours)

    def keyed(s, tri_map):
        """contour -> (its record without the first segment id, its segments as (old triangle, from, to) rows)"""
        out = {}
        for c in range(s.n_contours):
            lo, hi = s.contour_start[c], s.contour_start[c + 1]
            rows = [(int(tri_map[s.seg_tri[q]]),) + tuple(_bits(s.seg_points[q]).ravel().tolist()) for q in range(lo, hi)]
            out[c] = (tuple(s.counts[c, [0, 2, 3, 4, 5, 6]].tolist()), bool(s.closed[c]), rows)
        return out

    ka, kp = keyed(a, np.arange(len(perm))), keyed(p, perm)
    # a contour is named by its level and its set of (triangle, points) rows: the pairing of the two results
    name_a = {(v[0][0], frozenset(v[2])): c for c, v in ka.items()}
    assert len(name_a) == a.n_contours
    to_a = np.array([name_a[(v[0][0], frozenset(v[2]))] for v in kp.values()], np.int64)      # (KeyError: a contour has no partner)
    assert len(np.unique(to_a)) == a.n_contours
    for c, (rec, closed, rows) in kp.items():
        rec_a, closed_a, rows_a = ka[to_a[c]]
        assert rec == rec_a and closed == closed_a                                               # every integer
        if closed:                                                                               # the same cyclic sequence
            k = rows_a.index(rows[0])
            assert rows == rows_a[k:] + rows_a[:k]
    err, b = np.abs(p.sums - a.sums[to_a]), r["bound"][to_a]
    frac = float((err[b > 0] / b[b > 0]).max()) if (b > 0).any() else 0.0
    print(f"SECTIONS permuted {name}: largest fraction of the bound {frac:.4f}")
    assert (err <= b).all()


def test_rho2sdf_sections_option(pkg):
    X, IEN, rho = load_fixture("sphere")
    grid = pkg.Grid(X.min(0), X.max(0), 20, 3)
    opts = pkg.Rho2sdfOptions(threshold_density=0.5, rbf_grid="fine")
    info0 = {}
    plain = pkg.rho2sdf("t", X, IEN, rho, options=opts, sdf_grid=grid, info=info0)
    assert "sections" not in info0 and "surface" not in info0
    z = np.linspace(X[:, 2].min(), X[:, 2].max(), 9)[1:-1]
    info = {}
    got = pkg.rho2sdf("t", X, IEN, rho, options=opts, sdf_grid=grid, info=info, sections=((0.0, 0.0, 1.0), z))
    assert np.array_equal(got[0].view(np.uint32), plain[0].view(np.uint32)) and np.array_equal(_bits(got[3]), _bits(plain[3]))
    s = info["sections"]
    assert "surface" in info and _same(s, pkg.mesh_sections(*info["surface"], (0.0, 0.0, 1.0), z))
    assert s.n_contours >= 1 and s.closed.all() and (s.area > 0).all()
