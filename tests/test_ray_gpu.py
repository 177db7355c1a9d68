"""Ray queries on the GPU (r2s_mesh_index_raycast(_dev), surface_thickness(_dev), rho2sdf(thickness=True)) against the float64
restatement of the header's definition over ALL triangles (ray_ref64.raycast_brute): Float64 t, triangle and side are EQUAL on
every ray, Float32 output equals the restatement's value rounded once.  The shapes are the smallest at which the tree can
still go wrong."""
import ctypes

import numpy as np
import pytest

import mesh_dist_ref64 as M
import mesh_query_cases as C
import ray_cases as RC
import ray_ref64 as R
from conftest import load_fixture

pytestmark = pytest.mark.gpu
INF = np.inf


def _bits(a):
    return np.ascontiguousarray(a).view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same(label, got, want):
    """t bit-equal (NaN where NaN), triangle and side equal, on every ray"""
    (t, i, s), (tr, ir, sr) = got, want
    tr = tr.astype(t.dtype)
    bad = ~((t == tr) | (np.isnan(t) & np.isnan(tr))) | (i != ir) | (s != sr)
    print(f"RAY {label}: {len(t)} rays, {int(np.isfinite(tr).sum())} hits, {int(bad.sum())} differ")
    assert not bad.any(), (label, np.nonzero(bad)[0][:8], t[bad][:4], tr[bad][:4], i[bad][:4], ir[bad][:4])
    fin = np.isfinite(tr)
    assert np.array_equal(_bits(t[fin]), _bits(tr[fin])), label


def _surface(pkg, f, dims, origin, h, iso=0.0):
    L = pkg._lib
    a = np.ascontiguousarray(f)
    nv, nt = ctypes.c_int64(), ctypes.c_int64()
    L.check(L.lib().r2s_extract_isosurface(a.ctypes.data_as(ctypes.c_void_p), int(a.dtype == np.float32), (ctypes.c_int64 * 3)(*dims),
                                           (ctypes.c_double * 3)(*origin), h, iso, -1, None, 0, None, 0, ctypes.byref(nv), ctypes.byref(nt)))
    return pkg.api._last_isosurface()


_shared = {}


def _sphere(pkg, n):
    """the extracted surface of the n^3 sphere field -> (V, T, centre, radius)"""
    if ("sphere", n) not in _shared:
        h, origin = 0.25, (-3.0, 1.5, 0.25)
        r = 0.325 * (n - 1)
        V, T = _surface(pkg, C.sphere_field(n, r, np.float32), (n, n, n), origin, h)
        _shared[("sphere", n)] = (V, T, np.asarray(origin) + h * (n - 1) / 2, h * r)
    return _shared[("sphere", n)]


def _sphere_case(pkg):
    """the 33^3 sphere, 4096 rays of all families (not a multiple of 64: 4090) and the reference, computed once"""
    if "case" not in _shared:
        V, T, c, rad = _sphere(pkg, 33)
        o, d = RC.families(V, T, 700, 3, closed_centre=(c, rad))
        o, d = o[:4090], d[:4090]
        _shared["case"] = (V, T, o, d, R.raycast_brute(V, T, o, d))
    return _shared["case"]


def _cast(ix, o, d, **kw):
    return ix.raycast(o, d, want_index=True, want_side=True, **kw)


@pytest.mark.parametrize("n", [0, 1, 2, 3])
def test_first_triangles(pkg, n):
    V, T = C.first_triangles(n)
    o, d = RC.families(V, T, 151, 2)
    assert len(o) % 64 != 0
    with pkg.MeshIndex(V, T) as ix:
        want = R.raycast_brute(V, T, o, d)
        _same(f"{n} triangles", _cast(ix, o, d), want)
        _same(f"{n} triangles float32 out", _cast(ix, o, d, dtype=np.float32), want)
        o32, d32 = o.astype(np.float32), d.astype(np.float32)
        _same(f"{n} triangles float32 rays", _cast(ix, o32, d32), R.raycast_brute(V, T, o32.astype(np.float64), d32.astype(np.float64)))
        _same(f"{n} triangles window", _cast(ix, o, d, t_min=0.25, t_max=1.5), R.raycast_brute(V, T, o, d, 0.25, 1.5))
        assert len(ix.raycast(np.zeros((0, 3)), np.zeros((0, 3)))) == 0
    if n:
        assert np.isfinite(want[0]).sum() > 20
    else:
        fin = ~R.bad_rays(o, d)
        assert np.isposinf(want[0][fin]).all() and np.isnan(want[0][~fin]).all()


@pytest.mark.parametrize("case", ["planar", "degenerate", "cascade", "scale_mix"])
def test_meshes_that_stress_the_tree(pkg, case):
    V, T = getattr(C, case)()
    small = len(T) <= 1000
    o, d = RC.families(V, T, 300 if small else 450, 5)
    if case == "planar":                                             # rays in the plane z = 0.5 and across it
        oi, di = RC.uniform(V, 200, 6)
        oi[:, 2], di[:, 2] = 0.5, 0.0
        o, d = np.concatenate([o, oi]), np.concatenate([d, di])
    if not small:
        o, d = o[:4090], d[:4090]
    with pkg.MeshIndex(V, T) as ix:
        info = ix.info()
        got = _cast(ix, o, d)
        got32 = _cast(ix, o, d, dtype=np.float32)
    want = R.raycast_brute(V, T, o, d)
    _same(f"{case} (depth {info['depth']})", got, want)
    _same(f"{case} float32 out", got32, want)
    assert np.isfinite(want[0]).sum() > 50
    if case == "cascade":
        assert info["depth"] >= 12


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_sphere(pkg, dtype):
    V, T, o, d, want = _sphere_case(pkg)
    assert len(T) > 1000 and len(o) == 4090
    with pkg.MeshIndex(V, T) as ix:
        _same(f"sphere 33^3 {np.dtype(dtype).name} out", _cast(ix, o, d, dtype=dtype), want)
        if dtype == np.float32:
            o32, d32 = o.astype(np.float32), d.astype(np.float32)
            w32 = R.raycast_brute(V, T, o32.astype(np.float64), d32.astype(np.float64))
            _same("sphere 33^3 float32 rays", _cast(ix, o32, d32), w32)
            t = ix.raycast(o, d)                                     # the plain form returns t alone
            assert isinstance(t, np.ndarray) and np.array_equal(_bits(t), _bits(_cast(ix, o, d)[0]))
            t2, s2 = ix.raycast(o, d, want_side=True)
            assert s2.dtype == np.int8 and np.array_equal(s2, want[2])


@pytest.mark.parametrize("n", [17, 33])
def test_watertight_on_the_device(pkg, n):
    V, T, c, rad = _sphere(pkg, n)
    org = RC.inner_origins(c, rad, 7, 11)
    tg = np.concatenate([V.astype(np.float64), RC.edge_midpoints(V, T)])
    if n == 33:
        tg = tg[::4]
    o, d = RC.aimed(org, tg)
    with pkg.MeshIndex(V, T) as ix:
        t, i, s = _cast(ix, o, d)
    print(f"RAY watertight {n}^3: {len(o)} rays at {len(T)} triangles, misses {int(np.isinf(t).sum())}")
    assert np.isfinite(t).all() and (i >= 0).all() and (s == -1).all()


def test_order_independence(pkg):
    V, T, o, d, want = _sphere_case(pkg)
    rng = np.random.default_rng(12)
    perm = rng.permutation(len(T))
    with pkg.MeshIndex(V, T[perm]) as ix:
        t1, i1, s1 = _cast(ix, o, d)
    fin = np.isfinite(want[0])
    assert np.array_equal(_bits(t1[fin]), _bits(want[0][fin])) and np.array_equal(np.isnan(t1), np.isnan(want[0]))
    acc, tt, _ = R.pair_table(V, T, o[:512], d[:512])
    unique = (acc & (tt == want[0][:512, None])).sum(axis=1) == 1    # the minimum is attained by one triangle
    assert unique.sum() > 100
    assert np.array_equal(perm[i1[:512][unique]], want[1][:512][unique]) and np.array_equal(s1[:512][unique], want[2][:512][unique])
    pr = rng.permutation(len(o))
    with pkg.MeshIndex(V, T) as ix:
        t2, i2, s2 = _cast(ix, o[pr], d[pr])
    _same("permuted rays", (t2, i2, s2), tuple(w[pr] for w in want))


def test_dev_variant_second_stream_and_other_device_current(pkg):
    import torch
    V, T, o, d, want = _sphere_case(pkg)
    dev = torch.device("cuda", torch.cuda.current_device())
    to, td = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
    with pkg.MeshIndex(torch.from_numpy(V).to(dev), torch.from_numpy(T).to(dev)) as ix:
        for tdt, ndt in ((torch.float64, np.float64), (torch.float32, np.float32)):
            g = ix.raycast_dev(to, td, want_index=True, want_side=True, dtype=tdt)
            torch.cuda.synchronize()
            _same(f"_dev {np.dtype(ndt).name}", tuple(x.cpu().numpy() for x in g), want)
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        g = ix.raycast_dev(to, td, t_min=0.5, t_max=4.0, want_index=True, want_side=True, stream=st)
        st.synchronize()
        _same("_dev on a second stream", tuple(x.cpu().numpy() for x in g), R.raycast_brute(V, T, o, d, 0.5, 4.0))
        g32 = ix.raycast_dev(to.float(), td.float())
        h32 = ix.raycast(o.astype(np.float32), d.astype(np.float32))
        torch.cuda.synchronize()
        assert np.array_equal(_bits(g32.cpu().numpy()), _bits(h32))
        assert ix.raycast_dev(to[:0], td[:0]).numel() == 0
        if torch.cuda.device_count() > 1:
            other = (dev.index + 1) % torch.cuda.device_count()
            with torch.cuda.device(other):
                _same("host variant, another device current", _cast(ix, o, d), want)
                assert torch.cuda.current_device() == other
                with pytest.raises(pkg._lib.R2SError, match="device"):
                    ix.raycast_dev(to, td)
        else:
            print("RAY one device only: the host variant with another device current is not exercised")


def test_argument_errors_leave_the_outputs_untouched(pkg):
    import torch
    V, T = C.first_triangles(3)
    lib, L = pkg._lib.lib(), pkg._lib
    o, d = np.zeros((4, 3)), np.ones((4, 3))
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    with pkg.MeshIndex(V, T) as ix:
        h = ix._handle()
        out, tri, side = np.full(4, -7.0), np.full(4, -7, np.int32), np.full(4, -7, np.int8)
        args = lambda **k: [k.get("h", h), k.get("o", vp(o)), k.get("d", vp(d)), 0, k.get("n", 4), k.get("t0", 0.0), k.get("t1", INF), 0,   # noqa: E731
                            k.get("out", vp(out)), tri.ctypes.data_as(L.c_int32_p), vp(side)]
        for kw in (dict(h=None), dict(o=None), dict(d=None), dict(out=None), dict(n=-1), dict(t0=np.nan), dict(t1=np.nan),
                   dict(t0=1.0, t1=0.5)):
            assert lib.r2s_mesh_index_raycast(*args(**kw)) == -1, kw
        assert lib.r2s_mesh_index_raycast(*args(n=2 ** 31)) == -4
        assert lib.r2s_mesh_index_raycast(*args(n=0)) == 0
        assert (out == -7.0).all() and (tri == -7).all() and (side == -7).all()
        dev = torch.device("cuda", torch.cuda.current_device())
        to, td = torch.zeros((4, 3), dtype=torch.float64, device=dev), torch.ones((4, 3), dtype=torch.float64, device=dev)
        po = torch.full((4,), -7.0, dtype=torch.float64, device=dev)
        P = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
        for t0, t1, n in ((np.nan, 1.0, 4), (2.0, 1.0, 4), (0.0, 1.0, -1)):
            assert lib.r2s_mesh_index_raycast_dev(h, P(to), P(td), 0, n, t0, t1, 0, P(po), None, None, None) == -1
        assert lib.r2s_mesh_index_raycast_dev(h, None, P(td), 0, 4, 0.0, 1.0, 0, P(po), None, None, None) == -1
        torch.cuda.synchronize()
        assert (po.cpu().numpy() == -7.0).all()
        assert lib.r2s_mesh_index_raycast(*args()) == 0 and not (out == -7.0).any()


def test_surface_thickness_of_a_box(pkg):
    V, T = M.box_mesh((0, 0, 0), (1, 1, 0.25))
    th, tri, side = pkg.surface_thickness(V, T, np.array([[0, 0, 1.0]] * 8) * np.where(V[:, 2:3] > 0, 1.0, -1.0), skip=0.0625)
    top = V[:, 2] > 0
    assert np.array_equal(th, np.full(8, 0.25)) and (side == -1).all()
    v = V.astype(np.float64)
    assert (v[T[tri[top]]][:, :, 2] == 0.0).all() and (v[T[tri[~top]]][:, :, 2] == 0.25).all()   # the hit lies on the other face
    # the default normals point along the corner's diagonal: the ray leaves through another face, still from inside
    th2, tri2, side2 = pkg.surface_thickness(V, T, skip=0.0625)
    want = R.raycast_brute(V, T, v, -pkg.api._unit(pkg.vertex_normals(V, T)), t_min=0.0625)
    _same("box thickness, default normals", (th2, tri2, side2), want)
    assert np.isfinite(th2).all() and (side2 == -1).all()


def test_surface_thickness_of_the_sphere_host_and_device(pkg):
    import torch
    V, T, c, rad = _sphere(pkg, 33)
    skip = 0.125
    got = pkg.surface_thickness(V, T, skip=skip)
    d = -pkg.api._unit(pkg.vertex_normals(V, T))
    want = R.raycast_brute(V, T, V.astype(np.float64), d, t_min=skip)
    _same("sphere thickness", got, want)
    fin = np.isfinite(got[0])
    assert fin.mean() > 0.99 and abs(np.median(got[0][fin]) - 2 * rad) < 0.1 * rad and (got[2][fin] == -1).all()
    dev = torch.device("cuda", torch.cuda.current_device())
    tv, tt = torch.from_numpy(V).to(dev), torch.from_numpy(T).to(dev)
    g = pkg.surface_thickness_dev(tv, tt, skip=skip)
    _same("sphere thickness, device variant", tuple(x.cpu().numpy() for x in g), got)
    with pkg.MeshIndex(V, T) as ix:
        again = pkg.surface_thickness(V, T, skip=skip, index=ix)
        g2 = pkg.surface_thickness_dev(tv, tt, torch.from_numpy(pkg.vertex_normals(V, T)).to(dev), skip=skip, index=ix)
        torch.cuda.synchronize()
    _same("sphere thickness, given index", again, got)
    _same("sphere thickness, device variant with given normals and index", tuple(x.cpu().numpy() for x in g2), got)


def test_rho2sdf_thickness(pkg):
    X, IEN, rho = load_fixture("sphere")
    grid = pkg.Grid(X.min(0), X.max(0), 20, 3)
    opts = pkg.Rho2sdfOptions(threshold_density=0.5, rbf_grid="fine")
    info0 = {}
    plain = pkg.rho2sdf("t", X, IEN, rho, options=opts, sdf_grid=grid, info=info0)
    assert "thickness" not in info0 and "surface" not in info0
    info = {}
    got = pkg.rho2sdf("t", X, IEN, rho, options=opts, sdf_grid=grid, info=info, thickness=True)
    assert np.array_equal(_bits(plain[0]), _bits(got[0])) and np.array_equal(_bits(plain[3]), _bits(got[3]))
    assert np.array_equal(plain[1][0], got[1][0]) and plain[1][1:] == got[1][1:] and got[2] is grid
    skip = 0.5 * grid.cell_size / 2
    want = pkg.surface_thickness(*info["surface"], skip=skip)
    _same("rho2sdf thickness", info["thickness"], want)
    fin = np.isfinite(want[0])
    assert len(want[0]) == len(info["surface"][0]) > 100 and fin.mean() > 0.9 and (want[0][fin] >= skip).all()
    print(f"RAY rho2sdf sphere: median thickness {np.median(want[0][fin]):.4g} (cell {grid.cell_size:.4g})")
