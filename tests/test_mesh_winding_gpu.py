"""The winding entry points on the GPU (include/rho2sdf_hip.h, r2s_mesh_index_winding / _signed) against the numpy restatement of
tests/mesh_winding_ref.py on the named cases of tests/mesh_winding_cases.py: winding and crossings are EQUAL for every case and ray,
from the host, the device and the lattice entries; they follow a permutation of the triangles and of the points; all six rays
agree on closed meshes; the signed distance is the sign times MeshIndex.distance bit for bit; on the sphere iso-surfaces the sign
from the mesh reproduces r2s_redistance_full, the sign from the field, at EVERY lattice point; refusals; the index is unchanged."""
import ctypes

import numpy as np
import pytest

import mesh_winding_cases as C
import mesh_winding_ref as R

pytestmark = pytest.mark.gpu
vp = ctypes.c_void_p
RULES = ("positive", "nonzero", "odd")


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same(a, b):
    """bit equality; a NaN equals a NaN (its sign and payload are not part of any contract)"""
    return a.shape == b.shape and a.dtype == b.dtype and bool(((_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))).all())


@pytest.mark.parametrize("name", C.ANALYTIC)
def test_cases_equal_the_restatement(pkg, name):
    V, T = C.case(name)
    P = C.points(name)
    lat = C.lattice(name)
    nlat = int(np.prod(lat[0]))
    shape = (lat[0][2], lat[0][1], lat[0][0])
    with pkg.MeshIndex(V, T, device=0) as ix:
        for ray in R.RAYS:
            wn, nc = C.expected(name, ray)
            gw, gc = ix.winding(P, ray, want_crossings=True)
            assert gw.dtype == np.int32 and np.array_equal(gw, wn) and np.array_equal(gc, nc), (name, ray, "host")
            assert np.array_equal(ix.winding(P, ray), wn)                       # crossings_out may be NULL
            dw, dc = ix.winding_dev(_dev(P), ray, want_crossings=True)
            assert np.array_equal(dw.cpu().numpy(), wn) and np.array_equal(dc.cpu().numpy(), nc), (name, ray, "dev")
            lw, lc = ix.winding_lattice(lat, ray=ray, want_crossings=True)     # the lattice points are the first of P
            assert lw.shape == shape and np.array_equal(lw.ravel(), wn[:nlat]) and np.array_equal(lc.ravel(), nc[:nlat]), (name, ray, "lattice")
            lw, lc = ix.winding_lattice_dev(lat, ray=ray, want_crossings=True)
            assert np.array_equal(lw.cpu().numpy().ravel(), wn[:nlat]) and np.array_equal(lc.cpu().numpy().ravel(), nc[:nlat])
        for rule in RULES:
            wn, nc = C.expected(name, 2)
            assert np.array_equal(ix.contains(P, rule), R.inside(wn, nc, RULES.index(rule))), (name, rule)


def test_float32_points_and_point_counts(pkg):
    V, T = C.case("octahedra")
    P = C.points("octahedra")[4000:4065].astype(np.float32)
    with pkg.MeshIndex(V, T, device=0) as ix:
        for ray in (0, 4):
            wn, nc = R.winding_ref(V, T, P, ray)
            for n in (0, 1, 63, 64, 65):
                gw, gc = ix.winding(P[:n], ray, want_crossings=True)
                assert np.array_equal(gw, wn[:n]) and np.array_equal(gc, nc[:n]), (ray, n)
                dw = ix.winding_dev(_dev(P[:n]), ray)
                assert np.array_equal(dw.cpu().numpy(), wn[:n])


ROW_LATTICES = {   # odd dims, rows of 2 and of 65 on every axis, points that project onto vertices and edges
    "octahedra": [((21, 21, 21), (-2.5, -2.5, -2.5), 0.25), ((2, 65, 5), (-0.3, -2.4, -0.7), 0.075), ((65, 3, 2), (-2.4, -0.1, -0.2), 0.075),
                  ((7, 2, 65), (-1.0, 0.0, -2.4), 0.075)],
    "reversed_cube": [((7, 7, 7), (-0.5, -0.5, -0.5), 0.5), ((9, 2, 65), (-0.25, 0.5, -0.6), 0.05), ((65, 5, 2), (-0.6, 0.0, 1.0), 0.05)],
    "one_triangle": [((2, 65, 5), (-0.25, -0.25, -0.25), 0.04), ((3, 2, 2), (0.0, 0.0, 0.0), 1.0)],
    "empty": [((2, 3, 2), (0.0, 0.0, 0.0), 1.0)],
}


@pytest.mark.parametrize("name", sorted(ROW_LATTICES))
def test_rows_equal_points(pkg, name, monkeypatch):
    """the lattice entries by rows (mwn_rows_kernel + mwn_prefix_kernel, the default) == mwn_points_kernel on the same points, as
    an array and (R2S_WINDING_ROWS=0) on the lattice's 4x4x4 blocks == the restatement; winding, crossings and the signed distance
    of every rule, in both output types; for all six rays"""
    V, T = C.case(name)
    with pkg.MeshIndex(V, T, device=0) as ix:
        for lat in ROW_LATTICES[name]:
            P = C.lattice_points(lat)
            shape = (lat[0][2], lat[0][1], lat[0][0])
            for ray in R.RAYS:
                wn, nc = R.winding_ref(V, T, P, ray)
                pw, pc = ix.winding(P, ray, want_crossings=True)
                assert np.array_equal(pw, wn) and np.array_equal(pc, nc), (name, lat, ray, "points")
                monkeypatch.delenv("R2S_WINDING_ROWS", raising=False)
                rw, rc = ix.winding_lattice(lat, ray=ray, want_crossings=True)
                assert rw.shape == shape and np.array_equal(rw.ravel(), wn) and np.array_equal(rc.ravel(), nc), (name, lat, ray, "rows")
                assert np.array_equal(ix.winding_lattice(lat, ray=ray).ravel(), wn)
                rs = {(rule, dt): ix.signed_lattice(lat, rule=rule, ray=ray, want_index=True, dtype=dt)
                      for rule in RULES for dt in (np.float64, np.float32)}
                monkeypatch.setenv("R2S_WINDING_ROWS", "0")
                bw, bc = ix.winding_lattice(lat, ray=ray, want_crossings=True)
                assert np.array_equal(bw.ravel(), wn) and np.array_equal(bc.ravel(), nc), (name, lat, ray, "blocks")
                for (rule, dt), (sd, si) in rs.items():
                    bd, bi = ix.signed_lattice(lat, rule=rule, ray=ray, want_index=True, dtype=dt)
                    assert _same(sd, bd) and np.array_equal(si, bi), (name, lat, ray, rule, dt)
                    assert not np.signbit(sd[sd == 0]).any()
                monkeypatch.delenv("R2S_WINDING_ROWS")


@pytest.mark.parametrize("name", ["octahedra", "reversed_cube"])
def test_permutations(pkg, name):
    V, T = C.case(name)
    P = C.points(name)
    rng = np.random.default_rng(8)
    pt, pp = rng.permutation(len(T)), rng.permutation(len(P))
    with pkg.MeshIndex(V, T[pt], device=0) as ix:
        for ray in R.RAYS:
            wn, nc = C.expected(name, ray)
            gw, gc = ix.winding(P[pp], ray, want_crossings=True)
            assert np.array_equal(gw, wn[pp]) and np.array_equal(gc, nc[pp]), (name, ray)


@pytest.mark.parametrize("name", C.CLOSED)
def test_all_rays_agree_off_the_surface(pkg, name):
    V, T = C.case(name)
    P = C.points(name)
    off = ~C.on_surface(name, P)
    with pkg.MeshIndex(V, T, device=0) as ix:
        w = [ix.winding(P, ray) for ray in R.RAYS]
    for ray in R.RAYS:
        assert np.array_equal(w[ray][off], w[0][off]), (name, ray)
    assert np.array_equal(w[0][off], C.truth(name, P)[off])


@pytest.mark.parametrize("name", ["octahedra", "inward_cube", "reversed_cube", "empty"])
def test_signed_is_the_sign_times_the_distance(pkg, name):
    V, T = C.case(name)
    P = C.points(name)
    lat = C.lattice(name)
    nlat = int(np.prod(lat[0]))
    with pkg.MeshIndex(V, T, device=0) as ix:
        for dtype in (np.float64, np.float32):
            d, idx = ix.distance(P, want_index=True, dtype=dtype)
            dl, il = ix.lattice(lat, want_index=True, dtype=dtype)
            for rule in RULES:
                for ray in (2, 3):
                    wn, nc = C.expected(name, ray)
                    want = np.where(R.inside(wn, nc, RULES.index(rule)), d, -d) + dtype(0)     # (-0 -> +0)
                    s, si = ix.signed_distance(P, rule, ray, want_index=True, dtype=dtype)
                    assert _same(s, want) and np.array_equal(si, idx), (name, rule, ray, dtype)
                    assert np.isnan(s[-3:]).all() and not np.signbit(s[s == 0]).any()
                    assert _same(ix.signed_distance(P, rule, ray, dtype=dtype), want)
                    import torch
                    tdt = torch.float32 if dtype == np.float32 else torch.float64
                    sd, sdi = ix.signed_distance_dev(_dev(P), rule, ray, want_index=True, dtype=tdt)
                    assert _same(sd.cpu().numpy(), want) and np.array_equal(sdi.cpu().numpy(), idx)
                    sl, sli = ix.signed_lattice(lat, rule=rule, ray=ray, want_index=True, dtype=dtype)
                    assert _same(sl.ravel(), want[:nlat]) and np.array_equal(sli, il)
                    sld = ix.signed_lattice_dev(lat, rule=rule, ray=ray, dtype=tdt)
                    assert _same(sld.cpu().numpy().ravel(), want[:nlat])
            assert _same(dl.ravel(), d[:nlat])
        if name == "empty":
            assert (ix.signed_distance(P[:-3]) == -np.inf).all()
        dl64 = ix.lattice(lat).ravel()
    wn, nc = C.expected(name, 4)
    ins = R.inside(wn, nc, R.ODD)[:nlat]
    m = pkg.mesh_signed_distance(V, T, lat, rule="odd", ray=4, device=0)               # a tree built, used and dropped
    assert m.shape == (lat[0][2], lat[0][1], lat[0][0]) and _same(m.ravel(), np.where(ins, dl64, -dl64) + 0.0)
    md = pkg.mesh_signed_distance_dev(_dev(V), _dev(T), lat, rule="odd", ray=4)
    assert _same(md.cpu().numpy().ravel(), np.where(ins, dl64, -dl64) + 0.0)


@pytest.mark.parametrize("name", C.SPHERES)
def test_sphere_sign_from_the_mesh_equals_sign_from_the_field(pkg, name):
    """signed_lattice on the index of the extracted mesh == redistance_full of the field, bit for bit, at every lattice point, for
    every ray and rule; mesh_signed_distance equals the index path; winding and crossings equal the restatement for every ray (the whole lattice
    from the lattice entries and from the point entry, and seeded points off the lattice); the exact pair test agrees on a seeded sample of lattice points."""
    import torch
    s = C.sphere_case(pkg, name)
    V, T, lat, f = s["V"], s["T"], s["lattice"], s["f"]
    want = pkg.redistance_full(f, s["grid"], iso=0.0, device=0)
    assert want.dtype == np.float64 and (want > 0).any() and (want < 0).any()
    P = C.lattice_points(lat)
    rng = np.random.default_rng(17)
    lo, hi = V.min(axis=0).astype(np.float64), V.max(axis=0).astype(np.float64)
    Q = np.concatenate([rng.uniform(lo - 0.1, hi + 0.1, size=(400, 3)), P[rng.choice(len(P), 200, replace=False)]])
    with pkg.MeshIndex(V, T, device=0) as ix:
        for ray in R.RAYS:
            for rule in RULES:
                got = ix.signed_lattice(lat, rule=rule, ray=ray)
                assert _same(got, want), (name, ray, rule, int((_bits(got) != _bits(want)).sum()))
            wn, nc = R.winding_ref(V, T, Q, ray)
            gw, gc = ix.winding(Q, ray, want_crossings=True)
            assert np.array_equal(gw, wn) and np.array_equal(gc, nc), (name, ray)
            e, b = R.exact_disagreements(V, T, Q, ray)
            assert b == 0, (name, ray, e, b)
        dP = _dev(P)
        for ray in R.RAYS:
            wn, nc = R.winding_ref(V, T, P, ray)
            lw, lc = ix.winding_lattice(lat, ray=ray, want_crossings=True)
            assert np.array_equal(lw.ravel(), wn) and np.array_equal(lc.ravel(), nc), (name, ray)
            lw, lc = ix.winding_lattice_dev(lat, ray=ray, want_crossings=True)
            assert np.array_equal(lw.cpu().numpy().ravel(), wn) and np.array_equal(lc.cpu().numpy().ravel(), nc), (name, ray)
            pw, pc = ix.winding_dev(dP, ray, want_crossings=True)
            assert np.array_equal(pw.cpu().numpy(), wn) and np.array_equal(pc.cpu().numpy(), nc), (name, ray)
            assert np.array_equal(wn == 1, (f >= 0).ravel()) and np.array_equal(wn == 0, (f < 0).ravel())
        f32 = ix.signed_lattice(lat, dtype=np.float32)
        assert _same(f32, np.where(f >= 0, 1, -1).astype(np.float32) * np.abs(ix.lattice(lat, dtype=np.float32)))
    assert _same(pkg.mesh_signed_distance(V, T, lat, device=0), want)
    assert _same(pkg.mesh_signed_distance(V, T, s["grid"], rule="odd", ray=0), want)
    dv = pkg.mesh_signed_distance_dev(_dev(V), _dev(T), lat, ray=5, dtype=torch.float64)
    assert _same(dv.cpu().numpy(), want)


def test_index_is_unchanged(pkg):
    """distance and ray queries give their previous answers after the winding and signed calls"""
    V, T = C.case("octahedra")
    rng = np.random.default_rng(3)
    pts = rng.uniform(-2.5, 2.5, size=(500, 3))
    o, d = rng.uniform(-2.5, 2.5, size=(500, 3)), rng.normal(size=(500, 3))
    with pkg.MeshIndex(V, T, device=0) as ix:
        info = ix.info()
        d0, i0 = ix.distance(pts, want_index=True)
        r0 = ix.raycast(o, d, want_index=True, want_side=True)
        w0 = ix.winding(pts, 1, want_crossings=True)
        ix.signed_distance(pts)
        ix.signed_lattice(C.lattice("octahedra"))
        ix.winding_lattice(C.lattice("octahedra"), ray=3, want_crossings=True)
        ix.winding_dev(_dev(pts), 5)
        ix.winding_lattice_dev(C.lattice("octahedra"), ray=0)
        ix.signed_distance_dev(_dev(pts), "odd", 4)
        ix.signed_lattice_dev(C.lattice("octahedra"), rule="nonzero", ray=1)
        assert ix.info() == info
        d1, i1 = ix.distance(pts, want_index=True)
        r1 = ix.raycast(o, d, want_index=True, want_side=True)
        w1 = ix.winding(pts, 1, want_crossings=True)
    assert np.array_equal(d0, d1) and np.array_equal(i0, i1)
    assert all(np.array_equal(x, y) for x, y in zip(r0, r1)) and all(np.array_equal(x, y) for x, y in zip(w0, w1))


def test_argument_errors_leave_outputs_untouched(pkg):
    import torch
    L, lib = pkg._lib, pkg._lib.lib()
    V, T = C.case("cube22")
    P = np.ascontiguousarray(C.points("cube22")[:64])
    n = len(P)
    w, c, d = np.full(n, -7, np.int32), np.full(n, -7, np.int32), np.full(n, -7.0)
    pw, pc, pd, pp = w.ctypes.data_as(L.c_int32_p), c.ctypes.data_as(L.c_int32_p), d.ctypes.data_as(vp), P.ctypes.data_as(vp)
    dims, origin = (ctypes.c_int64 * 3)(4, 4, 4), (ctypes.c_double * 3)(0.0, 0.0, 0.0)
    bad_dims, bad_origin = (ctypes.c_int64 * 3)(4, 1, 4), (ctypes.c_double * 3)(0.0, float("nan"), 0.0)
    pv, pt = V.ctypes.data_as(L.c_float_p), T.ctypes.data_as(L.c_int32_p)
    bad_index = T.copy()
    bad_index[5, 1] = len(V)
    with pkg.MeshIndex(V, T, device=0) as ix:
        h = ix._handle()
        calls = [
            lambda: lib.r2s_mesh_index_winding(None, pp, 0, n, 2, pw, pc),
            lambda: lib.r2s_mesh_index_winding(h, None, 0, n, 2, pw, pc),
            lambda: lib.r2s_mesh_index_winding(h, pp, 0, n, 2, None, pc),
            lambda: lib.r2s_mesh_index_winding(h, pp, 0, -1, 2, pw, pc),
            lambda: lib.r2s_mesh_index_winding(h, pp, 0, n, 6, pw, pc),
            lambda: lib.r2s_mesh_index_winding(h, pp, 0, n, -1, pw, pc),
            lambda: lib.r2s_mesh_index_winding_lattice(h, dims, origin, 0.5, 6, pw, pc),
            lambda: lib.r2s_mesh_index_winding_lattice(h, bad_dims, origin, 0.5, 2, pw, pc),
            lambda: lib.r2s_mesh_index_winding_lattice(h, dims, bad_origin, 0.5, 2, pw, pc),
            lambda: lib.r2s_mesh_index_winding_lattice(h, dims, origin, 0.0, 2, pw, pc),
            lambda: lib.r2s_mesh_index_winding_lattice(None, dims, origin, 0.5, 2, pw, pc),
            lambda: lib.r2s_mesh_index_signed(h, pp, 0, n, 3, 2, 0, pd, pc),
            lambda: lib.r2s_mesh_index_signed(h, pp, 0, n, -1, 2, 0, pd, pc),
            lambda: lib.r2s_mesh_index_signed(h, pp, 0, n, 0, 7, 0, pd, pc),
            lambda: lib.r2s_mesh_index_signed(h, pp, 0, n, 0, 2, 0, None, pc),
            lambda: lib.r2s_mesh_index_signed_lattice(h, dims, origin, 0.5, 3, 2, 0, pd, pc),
            lambda: lib.r2s_mesh_index_signed_lattice(h, dims, origin, 0.5, 0, 6, 0, pd, pc),
            lambda: lib.r2s_mesh_index_signed_lattice(h, dims, origin, float("inf"), 0, 2, 0, pd, pc),
            lambda: lib.r2s_mesh_signed_distance(pv, len(V), pt, len(T), dims, origin, 0.5, 3, 2, 0, 0, pd),
            lambda: lib.r2s_mesh_signed_distance(pv, len(V), pt, len(T), dims, origin, 0.5, 0, 6, 0, 0, pd),
            lambda: lib.r2s_mesh_signed_distance(pv, len(V), pt, len(T), bad_dims, origin, 0.5, 0, 2, 0, 0, pd),
            lambda: lib.r2s_mesh_signed_distance(pv, len(V), None, len(T), dims, origin, 0.5, 0, 2, 0, 0, pd),
            lambda: lib.r2s_mesh_signed_distance(pv, len(V), bad_index.ctypes.data_as(L.c_int32_p), len(T), dims, origin, 0.5, 0, 2, 0, 0, pd),
        ]
        for k, call in enumerate(calls):
            assert call() == -1, k
        assert (w == -7).all() and (c == -7).all() and (d == -7.0).all()
        assert lib.r2s_mesh_index_winding(h, None, 0, 0, 2, None, None) == 0           # n == 0 succeeds and touches nothing
        dw, dd, dP = _dev(w), _dev(d), _dev(P)
        st = vp(torch.cuda.current_stream().cuda_stream)
        dV, dB = _dev(V), _dev(bad_index)
        dev_calls = [
            lambda: lib.r2s_mesh_index_winding_dev(None, vp(dP.data_ptr()), 0, n, 2, vp(dw.data_ptr()), None, st),
            lambda: lib.r2s_mesh_index_winding_dev(h, vp(dP.data_ptr()), 0, n, 6, vp(dw.data_ptr()), None, st),
            lambda: lib.r2s_mesh_index_winding_lattice_dev(h, dims, origin, 0.5, -2, vp(dw.data_ptr()), None, st),
            lambda: lib.r2s_mesh_index_signed_dev(h, vp(dP.data_ptr()), 0, n, 5, 2, 0, vp(dd.data_ptr()), None, st),
            lambda: lib.r2s_mesh_index_signed_lattice_dev(h, bad_dims, origin, 0.5, 0, 2, 0, vp(dd.data_ptr()), None, st),
            lambda: lib.r2s_mesh_signed_distance_dev(vp(dV.data_ptr()), len(V), vp(dB.data_ptr()), len(T), dims, origin, 0.5, 0, 2, 0,
                                                     vp(dd.data_ptr()), st),
            lambda: lib.r2s_mesh_signed_distance_dev(vp(dV.data_ptr()), len(V), vp(dV.data_ptr()), len(T), dims, origin, 0.5, 0, 9, 0,
                                                     vp(dd.data_ptr()), st),
        ]
        for k, call in enumerate(dev_calls):
            assert call() == -1, k
        torch.cuda.synchronize()
        assert (dw.cpu().numpy() == -7).all() and (dd.cpu().numpy() == -7.0).all()
        if torch.cuda.device_count() > 1:                  # the index lives on device 0
            with torch.cuda.device(1):
                d1w, d1p = torch.full((n,), -7, dtype=torch.int32, device="cuda:1"), torch.zeros((n, 3), dtype=torch.float64, device="cuda:1")
                assert lib.r2s_mesh_index_winding_dev(h, vp(d1p.data_ptr()), 0, n, 2, vp(d1w.data_ptr()), None,
                                                      vp(torch.cuda.current_stream().cuda_stream)) == -1
                assert (d1w.cpu().numpy() == -7).all()
    with pytest.raises(pkg._lib.R2SError):
        pkg.mesh_signed_distance(V, T, C.lattice("cube22"), rule="even")
    with pkg.MeshIndex(V, T, device=0) as ix:
        for bad in ("even", 5, -1):
            with pytest.raises(pkg._lib.R2SError):
                ix.contains(P, bad)
        assert np.array_equal(ix.contains(P, 2), ix.contains(P, "odd"))
