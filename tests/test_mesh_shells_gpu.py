"""The mesh shells on the GPU (r2s_mesh_shells, r2s_mesh_shells_dev, rho2sdf(shells=True)) against the restatement of
tests/mesh_shells_ref64.py on every case of tests/mesh_shells_cases.py: shell_of_tri, every integer record, the totals and the
reference point exactly, every Float64 entry within

    bound(s) = (n_tris(s) + K) * 2^-53 * T(s)

(K and T as in the restatement; tests/test_mesh_shells_cpu.py holds the restatement itself to that bound against an exact
evaluation).  Each case prints the largest fraction of the bound used as a "SHELLS ..." line."""
import ctypes

import numpy as np
import pytest

import mesh_shells_cases as C
import mesh_shells_ref64 as M
from conftest import load_fixture

pytestmark = pytest.mark.gpu

_ref = {}


def _restated(name):
    """the restatement of a case, computed once and left unchanged"""
    if name not in _ref:
        _ref[name] = M.shells(*C.case(name))
    return _ref[name]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _same(a, b):
    """two results bit for bit"""
    return (np.array_equal(a.counts, b.counts) and np.array_equal(_bits(a.sums), _bits(b.sums)) and np.array_equal(a.totals, b.totals)
            and np.array_equal(_bits(a.ref_point), _bits(b.ref_point))
            and np.array_equal(np.asarray(a.shell_of_tri), np.asarray(b.shell_of_tri)))


def _check(label, s, r, factor=1.0):
    assert np.array_equal(s.shell_of_tri, r["shell_of_tri"]), label
    assert np.array_equal(s.counts, r["counts"]), label
    assert np.array_equal(s.totals, r["totals"]), label
    assert np.array_equal(_bits(s.ref_point), _bits(r["ref_point"])), label
    err, b = np.abs(s.sums - r["sums"]), factor * r["bound"]
    frac = float((err[b > 0] / b[b > 0]).max()) if (b > 0).any() else 0.0
    print(f"SHELLS {label}: {len(s.shell_of_tri)} triangles, {s.n_shells} shells, largest fraction of the bound {frac:.4f}")
    assert (err <= b).all(), (label, frac)


def _extract(pkg, name):
    L = pkg._lib
    n, f = C.fields()[name]
    f = np.ascontiguousarray(f, np.float32)
    nv, nt = ctypes.c_int64(), ctypes.c_int64()
    L.check(L.lib().r2s_extract_isosurface(f.ctypes.data_as(ctypes.c_void_p), 1, (ctypes.c_int64 * 3)(n, n, n),
                                           (ctypes.c_double * 3)(*C.ORIGIN), C.SPACING, 0.0, -1, None, 0, None, 0, ctypes.byref(nv),
                                           ctypes.byref(nt)))
    return pkg.api._last_isosurface()


@pytest.mark.parametrize("name", C.ALL)
def test_equal_to_the_restatement(pkg, name):
    V, T = C.case(name)
    if name in C.EXTRACTED:   # the recorded mesh is the one the library extracts
        Vx, Tx = _extract(pkg, name)
        assert np.array_equal(Vx.view(np.uint32), V.view(np.uint32)) and np.array_equal(Tx, T)
    s = pkg.mesh_shells(V, T)
    _check(name, s, _restated(name))


def test_what_the_cases_must_show(pkg):
    sh = {name: pkg.mesh_shells(*C.case(name)) for name in C.ALL if not name.startswith("ribbon_")}
    assert sh["empty"].n_shells == 0 and sh["empty"].totals.tolist() == [0] * 8 and (sh["empty"].ref_point == 0).all()
    s = sh["one_triangle"]
    assert s.n_shells == 1 and s.n_boundary.tolist() == [3] and not s.closed[0]
    s = sh["all_collapsed"]
    assert s.n_shells == 0 and (s.shell_of_tri == -1).all() and s.totals[:3].tolist() == [0, 4, 4]
    s = sh["tetrahedron"]
    assert s.closed.tolist() == [True] and s.euler.tolist() == [2] and s.genus.tolist() == [0]
    assert (s.ref_point == 30.0).all()
    # closed forms of the corner tetrahedron of side L = 60 about (L/2, L/2, L/2): V = L^3/6, M_i = L^4/24 - (L/2) V,
    # P_ii = L^5/60 - L * L^4/24 + (L/2)^2 V, P_ij = L^5/120 - L * L^4/24 + (L/2)^2 V; every term is an integer
    assert _bits(s.sums[0, 1:]).tolist() == _bits(np.array([36000.0] + [-540000.0] * 3 + [12960000.0] * 3 + [6480000.0] * 3)).tolist()
    assert (s.centroid == 15.0).all() and not s.is_void[0]
    s = sh["cube_with_void"]
    assert s.n_shells == 2 and s.closed.all() and s.is_void.tolist() == [False, True] and s.area.tolist() == [24.0, 6.0]
    s = sh["two_tets_sharing_vertex"]
    assert s.n_shells == 2 and s.n_verts.tolist() == [4, 4] and s.totals[7] == 7
    s = sh["three_on_edge"]
    assert s.n_shells == 1 and s.n_nonmanifold.tolist() == [1] and s.n_boundary.tolist() == [6]
    s = sh["triangle_twice"]
    assert s.n_shells == 1 and s.n_flipped.tolist() == [3] and s.n_edges.tolist() == [3] and not s.closed[0]
    s = sh["cube_one_reversed"]
    assert s.n_flipped.tolist() == [3] and s.n_boundary.tolist() == [0] and not s.closed[0] and s.genus.tolist() == [-1]
    s = sh["torus"]
    assert s.closed.tolist() == [True] and s.euler.tolist() == [0] and s.genus.tolist() == [1]
    s = sh["sphere33"]
    assert s.n_shells == 1 and s.closed[0] and s.genus[0] == 0 and s.totals[4:7].tolist() == [0, 0, 0] and s.volume[0] > 0
    s = sh["nested41"]
    assert s.n_shells == 3 and s.closed.all() and (np.sign(s.volume) == [1, -1, 1]).all() and s.is_void.tolist() == [False, True, False]
    s = sh["gyroid17"]
    assert s.n_boundary.sum() > 0 and not s.closed.any()
    s = sh["noise24_closed"]
    assert s.n_shells >= 200 and s.closed.all()
    assert sh["noise24_open"].n_boundary.sum() > 0
    s = sh["ribbon"]
    assert s.n_shells == 1 and (s.shell_of_tri == 0).all()
    assert sh["disjoint"].n_shells == 3000
    assert (sh["fans"].n_tris == np.arange(1, 401)).all()


@pytest.mark.parametrize("name", ["ribbon_reversed", "ribbon_shuffled"])
def test_ribbon_in_other_orders_is_one_shell(pkg, name):
    s = pkg.mesh_shells(*C.case(name))
    assert s.n_shells == 1 and (s.shell_of_tri == 0).all() and s.n_tris.tolist() == [20000]


def _dev(pkg, V, T, capacity=0):
    import torch
    v, t = torch.from_numpy(np.ascontiguousarray(V)).cuda(), torch.from_numpy(np.ascontiguousarray(T)).cuda()
    s = pkg.mesh_shells_dev(v, t, capacity=capacity)
    s.shell_of_tri = s.shell_of_tri.cpu().numpy()
    return s


@pytest.mark.parametrize("name", ["noise24_closed", "noise24_open", "ribbon"])
def test_reproducible_bit_for_bit(pkg, name):
    V, T = C.case(name)
    a, b = pkg.mesh_shells(V, T), pkg.mesh_shells(V, T)
    assert _same(a, b)
    assert _same(a, _dev(pkg, V, T)) and _same(a, _dev(pkg, V, T, capacity=a.n_shells + 5))
    pkg._lib.lib().r2s_release_cache()                      # fresh work buffers
    assert _same(a, pkg.mesh_shells(V, T))


@pytest.mark.parametrize("name", ["noise24_closed", "noise24_open", "ribbon"])
def test_permutation_of_the_triangles(pkg, name):
    V, T = C.case(name)
    (_, Tp), perm = C.permuted((V, T), 33)
    a, p = pkg.mesh_shells(V, T), pkg.mesh_shells(V, Tp)
    r = _restated(name)
    assert a.n_shells == p.n_shells and np.array_equal(a.totals, p.totals)
    # shell k of the permuted mesh is the shell `to_a[k]` of the original one
    inv = np.empty_like(perm)
    inv[perm] = np.arange(len(perm))
    to_a = a.shell_of_tri[perm[p.first_tri]]
    assert len(np.unique(to_a)) == a.n_shells
    assert np.array_equal(to_a[p.shell_of_tri], a.shell_of_tri[perm])                   # the partition
    assert np.array_equal(p.counts[:, 1:], a.counts[to_a, 1:])                          # every integer
    first = np.array([inv[np.nonzero(a.shell_of_tri == k)[0]].min() for k in to_a]) if a.n_shells < 5000 else None
    assert first is None or np.array_equal(p.first_tri, first)                          # first_tri after mapping
    err, b = np.abs(p.sums - a.sums[to_a]), 2.0 * r["bound"][to_a]
    frac = float((err[b > 0] / b[b > 0]).max()) if (b > 0).any() else 0.0
    print(f"SHELLS permuted {name}: largest fraction of twice the bound {frac:.4f}")
    assert (err <= b).all()


def test_dev_capacity_zero_leaves_the_tables_untouched(pkg):
    import torch
    L = pkg._lib
    V, T = C.case("cube_with_void")
    v, t = torch.from_numpy(V).cuda(), torch.from_numpy(T).cuda()
    counts = torch.full((2, 8), -7, dtype=torch.int64, device="cuda")
    sums = torch.full((2, 11), -7.0, dtype=torch.float64, device="cuda")
    n, ref, tot = ctypes.c_int64(), np.zeros(3), np.zeros(8, np.int64)
    vp = ctypes.c_void_p
    args = (vp(v.data_ptr()), len(V), vp(t.data_ptr()), len(T), None, vp(counts.data_ptr()), vp(sums.data_ptr()))
    tail = (ctypes.byref(n), ref.ctypes.data_as(L.c_double_p), tot.ctypes.data_as(L.c_int64_p), None)
    for cap in (0, 1):
        L.check(L.lib().r2s_mesh_shells_dev(*args, cap, *tail))
        assert n.value == 2 and tot.tolist() == [2, 24, 0, 36, 0, 0, 0, 16] and (ref == 1.0).all()
        assert (counts == -7).all() and (sums == -7.0).all()
    L.check(L.lib().r2s_mesh_shells_dev(*args, 2, *tail))
    assert counts.cpu().numpy()[:, :2].tolist() == [[0, 12], [12, 12]] and sums.cpu().numpy()[:, 1].tolist() == [8.0, -1.0]


def test_bad_mesh_is_refused_with_the_outputs_untouched(pkg):
    import torch
    L = pkg._lib
    V, T = C.case("cube_with_void")
    Tb, Vb = T.copy(), V.copy()
    Tb[5, 2] = len(V)
    Vb[3, 1] = np.nan
    vp = ctypes.c_void_p
    for Vx, Tx in ((V, Tb), (Vb, T)):
        sot = np.full(len(T), -7, np.int32)
        n, ref, tot = ctypes.c_int64(-7), np.full(3, -7.0), np.full(8, -7, np.int64)
        rc = L.lib().r2s_mesh_shells(Vx.ctypes.data_as(L.c_float_p), len(Vx), Tx.ctypes.data_as(L.c_int32_p), len(Tx), -1,
                                     sot.ctypes.data_as(L.c_int32_p), ctypes.byref(n), ref.ctypes.data_as(L.c_double_p),
                                     tot.ctypes.data_as(L.c_int64_p))
        assert rc == -1 and (sot == -7).all() and n.value == -7 and (ref == -7.0).all() and (tot == -7).all()
        v, t = torch.from_numpy(Vx).cuda(), torch.from_numpy(Tx).cuda()
        dsot = torch.full((len(T),), -7, dtype=torch.int32, device="cuda")
        counts = torch.full((4, 8), -7, dtype=torch.int64, device="cuda")
        sums = torch.full((4, 11), -7.0, dtype=torch.float64, device="cuda")
        rc = L.lib().r2s_mesh_shells_dev(vp(v.data_ptr()), len(Vx), vp(t.data_ptr()), len(Tx), vp(dsot.data_ptr()), vp(counts.data_ptr()),
                                         vp(sums.data_ptr()), 4, ctypes.byref(n), ref.ctypes.data_as(L.c_double_p),
                                         tot.ctypes.data_as(L.c_int64_p), None)
        assert rc == -1 and n.value == -7 and (ref == -7.0).all() and (tot == -7).all()
        assert (dsot == -7).all() and (counts == -7).all() and (sums == -7.0).all()


def test_rho2sdf_shells_option(pkg):
    X, IEN, rho = load_fixture("sphere")
    grid = pkg.Grid(X.min(0), X.max(0), 20, 3)
    opts = pkg.Rho2sdfOptions(threshold_density=0.5, rbf_grid="fine")
    info0 = {}
    plain = pkg.rho2sdf("t", X, IEN, rho, options=opts, sdf_grid=grid, info=info0)
    assert "shells" not in info0 and "surface" not in info0
    info = {}
    got = pkg.rho2sdf("t", X, IEN, rho, options=opts, sdf_grid=grid, info=info, shells=True)
    assert np.array_equal(got[0].view(np.uint32), plain[0].view(np.uint32)) and np.array_equal(_bits(got[3]), _bits(plain[3]))
    assert got[1][1] == plain[1][1] and got[1][2] == plain[1][2] and (got[1][0] == plain[1][0]).all()
    assert "surface" in info and _same(info["shells"], pkg.mesh_shells(*info["surface"]))
    assert info["shells"].n_shells >= 1 and info["shells"].totals[1] == len(info["surface"][1])
