"""The mesh index on the GPU (r2s_mesh_index_*, r2s_redistance_full, surface_deviation, rho2sdf(signed_distance, deviation))
against the float64 restatement of the header's definition over ALL triangles (mesh_dist_ref64.distance_brute).  Every point
is compared:

    |out - d_ref| <= u |d_ref| + K 2^-52 L      u = 2^-24 (Float32 output) or 2^-53, K as in the helper, L the largest
                                                 absolute coordinate over the (finite) points and the vertices,

and the reference's distance to the reported triangle is within the same bound of d_ref.  Each test prints the largest fraction
of the bound used as a "MESHQ ..." line.  The shapes are the smallest at which the tree can still go wrong."""
import ctypes
import functools

import numpy as np
import pytest

import iso_ref as R
import mesh_dist_ref64 as M
import mesh_query_cases as C
from conftest import load_fixture

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a).view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _scale(V, P):
    fin = np.isfinite(P).all(axis=1)
    L = float(np.abs(P[fin]).max()) if fin.any() else 0.0
    return max(L, float(np.abs(np.asarray(V, np.float64)).max()) if len(V) else 0.0)


def _check(label, V, T, P, d, idx, ref=None):
    """the bound on every point and the closest-triangle rule -> the reference (d_ref, idx_ref)"""
    P = np.asarray(P, np.float64).reshape(-1, 3)
    d, idx = np.asarray(d).ravel(), np.asarray(idx).ravel()
    fin = np.isfinite(P).all(axis=1)
    assert np.isnan(d[~fin]).all() and (idx[~fin] == -1).all(), label
    if ref is None:
        ref = M.distance_brute(V, T, P[fin])
    dr, ir = ref
    L = _scale(V, P)
    if len(T) == 0:
        assert np.isposinf(d[fin]).all() and (idx[fin] == -1).all(), label
        print(f"MESHQ {label}: {int(fin.sum())} points, no triangles")
        return ref
    b = M.bound(dr, L, d.dtype)
    frac = np.abs(d[fin].astype(np.float64) - dr) / b
    assert ((idx[fin] >= 0) & (idx[fin] < len(T))).all(), label
    dt = M.distance_to_given(V, T, P[fin], idx[fin])
    fi = np.abs(dt - dr) / M.bound(dr, L, np.float64)
    print(f"MESHQ {label}: {int(fin.sum())} points, {len(T)} triangles, largest fraction of the bound {frac.max():.3f}, "
          f"of the reported triangle {fi.max():.3f} (L = {L:.4g})")
    assert frac.max() <= 1.0, (label, int((frac > 1).sum()), frac.max())
    assert fi.max() <= 1.0, (label, "the reported triangle is not a closest one", int((fi > 1).sum()))
    return ref


def _surface(pkg, f, dims, origin, h, iso=0.0):
    """the mesh r2s_extract_isosurface returns for the lattice (dims, origin, h)"""
    L = pkg._lib
    a = np.ascontiguousarray(f)
    nv, nt = ctypes.c_int64(), ctypes.c_int64()
    L.check(L.lib().r2s_extract_isosurface(a.ctypes.data_as(ctypes.c_void_p), int(a.dtype == np.float32), (ctypes.c_int64 * 3)(*dims),
                                           (ctypes.c_double * 3)(*origin), h, iso, -1, None, 0, None, 0, ctypes.byref(nv), ctypes.byref(nt)))
    return pkg.api._last_isosurface()


def _query(pkg, V, T, P, dtype=np.float64):
    with pkg.MeshIndex(V, T) as ix:
        return ix.distance(P, want_index=True, dtype=dtype)


_shared = {}


def _sphere_case(pkg):
    """the extracted surface of a 33^3 sphere field, its lattice and the point sets, with the float64 reference computed once"""
    if "sphere" not in _shared:
        n, h, origin = 33, 0.25, (-3.0, 1.5, 0.25)
        f = C.sphere_field(n, 5.2, np.float32)
        grid = ((n, n, n), origin, h)
        V, T = _surface(pkg, f, (n, n, n), origin, h)
        lo, hi = np.array(origin), np.array(origin) + h * (n - 1)
        P = np.concatenate([M.lattice_points((n, n, n), origin, h), C.box_points(lo, hi, 4096, 3), C.far_points(lo, hi, 512, 5),
                            V.astype(np.float64), C.bad_rows()])
        fin = np.isfinite(P).all(axis=1)
        _shared["sphere"] = (f, grid, V, T, P, M.distance_brute(V, T, P[fin]))
    return _shared["sphere"]


@pytest.mark.parametrize("n", [0, 1, 2, 3])
def test_first_triangles(pkg, n):
    V, T = C.first_triangles(n)
    P = np.concatenate([C.box_points((-1, -1, -1), (2, 2, 2), 300, 2), V.astype(np.float64), C.bad_rows()])
    with pkg.MeshIndex(V, T) as ix:
        info = ix.info()
        for dtype in (np.float64, np.float32):
            d, idx = ix.distance(P, want_index=True, dtype=dtype)
            _check(f"{n} triangles {np.dtype(dtype).name}", V, T, P, d, idx)
        d32 = ix.distance(P.astype(np.float32))
        _check(f"{n} triangles float32 points", V, T, P.astype(np.float32).astype(np.float64), d32, ix.distance(P.astype(np.float32), True)[1])
        assert len(ix.distance(np.zeros((0, 3)))) == 0
    assert info["n_tris"] == n and info["n_nodes"] == max(2 * n - 1, 0) and info["depth"] == (0, 0, 1, 2)[n]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_sphere(pkg, dtype):
    f, grid, V, T, P, ref = _sphere_case(pkg)
    assert len(T) > 500
    with pkg.MeshIndex(V, T) as ix:
        d, idx = ix.distance(P, want_index=True, dtype=dtype)
        info = ix.info()
        dl, il = ix.lattice(grid, want_index=True, dtype=dtype)
    assert d.dtype == dtype and 0 < info["depth"] <= 64 and info["device_bytes"] >= 64 * (len(T) - 1)
    _check(f"sphere 33^3 {np.dtype(dtype).name}", V, T, P, d, idx, ref)
    nl = 33 ** 3
    on = slice(nl + 4096 + 512, nl + 4096 + 512 + len(V))
    assert (d[on] == 0.0).all()                                       # every vertex lies on the mesh
    assert np.array_equal(_bits(dl.ravel()), _bits(d[:nl])) and np.array_equal(il.ravel(), idx[:nl])


@functools.lru_cache(maxsize=None)
def _gyroid(n, period):
    return R.gyroid(n, period).ravel(), (n, n, n), (-1.0, -1.0, -1.0), 2.0 / (n - 1)


def test_gyroid_lattice_point_and_banded_entries_agree(pkg):
    f, dims, origin, h = _gyroid(41, 13)
    lat = (dims, origin, h)
    V, T = _surface(pkg, f, dims, origin, h)
    assert len(T) > 10000
    P = M.lattice_points(dims, origin, h)
    band = 3.0 * h
    with pkg.MeshIndex(V, T) as ix:
        dl, il = ix.lattice(lat, want_index=True)
        dp, ip = ix.distance(P, want_index=True)
        dl32 = ix.lattice(lat, dtype=np.float32)
    assert np.array_equal(_bits(dl.ravel()), _bits(dp)) and np.array_equal(il.ravel(), ip)
    assert np.array_equal(_bits(dl32), _bits(dl.astype(np.float32)))
    db, ib = pkg.mesh_distance(V, T, lat, band, want_index=True)
    inb = db.ravel() < band
    assert inb.sum() > 20000
    assert np.array_equal(_bits(db.ravel()[inb]), _bits(dp[inb])) and np.array_equal(ib.ravel()[inb], ip[inb])
    assert (dp[~inb] >= band).all()
    # a sample against the restatement over all triangles
    pick = np.random.default_rng(3).choice(len(P), 256, replace=False)
    _check("gyroid 41^3 sample", V, T, P[pick], dp[pick], ip[pick])


@pytest.mark.parametrize("case", ["planar", "degenerate", "plane_through_lattice"])
def test_degenerate_geometry(pkg, case):
    if case == "plane_through_lattice":
        dims, origin, h = (12, 9, 7), (0.5, -0.25, 2.0), 0.5
        k, j, i = np.meshgrid(np.arange(7.0), np.arange(9.0), np.arange(12.0), indexing="ij")
        hi = [origin[a] + h * (dims[a] - 1) for a in range(3)]
        V, T = _surface(pkg, (i - 5.0).ravel(), dims, origin, h)
        P = np.concatenate([M.lattice_points(dims, origin, h), C.box_points(origin, hi, 500, 1)])
    else:
        V, T = getattr(C, case)()
        lo, hi = V.min(0) - 0.5, V.max(0) + 0.5
        P = np.concatenate([C.box_points(lo, hi, 1500, 1), C.far_points(lo, hi, 64, 2), V.astype(np.float64), C.bad_rows()])
    for dtype in (np.float64, np.float32):
        d, idx = _query(pkg, V, T, P, dtype)
        ref = _check(f"{case} {np.dtype(dtype).name}", V, T, P, d, idx, _shared.get(("deg", case)))
        _shared[("deg", case)] = ref


def test_duplicates(pkg):
    f, grid, V, T, P, ref = _sphere_case(pkg)
    Q = P[33 ** 3:33 ** 3 + 4096]
    d1, i1 = _query(pkg, V, T, Q)
    d2, i2 = _query(pkg, V, np.concatenate([T, T]), Q)
    assert np.array_equal(_bits(d1), _bits(d2)) and (i2 < len(T)).all() and np.array_equal(i1, i2)
    V1, T1 = C.first_triangles(1)
    d, idx = _query(pkg, V1, np.repeat(T1, 4096, axis=0), Q)
    assert (idx == 0).all()
    _check("4096 copies of one triangle", V1, T1, Q, d, idx)


def test_cascade_deep_tree(pkg):
    V, T = C.cascade()
    P = np.concatenate([C.box_points((-0.5, -0.5, -0.5), (1.5, 1.0, 1.0), 1200, 4), V[::5].astype(np.float64)])
    with pkg.MeshIndex(V, T) as ix:
        info = ix.info()
        d, idx = ix.distance(P, want_index=True)
    print(f"MESHQ cascade: depth {info['depth']}, {info['n_nodes']} nodes")
    assert 12 <= info["depth"] <= 64                                  # deeper than a balanced tree (11), within the stack
    _check("cascade", V, T, P, d, idx)


def test_scale_mix(pkg):
    V, T = C.scale_mix()
    P = np.concatenate([C.box_points((0, 0, 0), (1, 1, 1), 1000, 6), C.box_points((0.3, 0.3, 0.3), (0.7, 0.7, 0.7), 500, 7)])
    d, idx = _query(pkg, V, T, P)
    _check("scale mix", V, T, P, d, idx)
    assert (idx < 2).any() and (idx >= 2).any()


def test_order_independence(pkg):
    f, grid, V, T, P, ref = _sphere_case(pkg)
    Q = P[33 ** 3:33 ** 3 + 4096 + 512]
    rq = (ref[0][33 ** 3:33 ** 3 + 4608], ref[1][33 ** 3:33 ** 3 + 4608])
    rng = np.random.default_rng(12)
    perm = rng.permutation(len(T))
    d0, i0 = _query(pkg, V, T, Q)
    d1, i1 = _query(pkg, V, T[perm], Q)
    assert np.array_equal(_bits(d0), _bits(d1))
    _check("permuted triangles", V, T[perm], Q, d1, i1, (rq[0], None))
    pp = rng.permutation(len(Q))
    d2, i2 = _query(pkg, V, T, Q[pp])
    assert np.array_equal(_bits(d2), _bits(d0[pp])) and np.array_equal(i2, i0[pp])


def test_host_and_dev_variants_and_lifetimes(pkg):
    import torch
    f, grid, V, T, P, ref = _sphere_case(pkg)
    Q = P[33 ** 3:33 ** 3 + 4096]
    dev = torch.device("cuda", torch.cuda.current_device())
    a = pkg.MeshIndex(V, T)
    b = pkg.MeshIndex(torch.from_numpy(V).to(dev), torch.from_numpy(T).to(dev))
    V3, T3 = C.first_triangles(3)
    c = pkg.MeshIndex(V3, T3)
    try:
        assert a.info() == b.info()
        want, wi = a.distance(Q, want_index=True)
        for dt, tdt in ((np.float64, torch.float64), (np.float32, torch.float32)):
            hd, hi = a.distance(Q, want_index=True, dtype=dt)
            gd, gi = b.distance_dev(torch.from_numpy(Q).to(dev), want_index=True, dtype=tdt)
            assert np.array_equal(_bits(hd), _bits(gd.cpu().numpy())) and np.array_equal(hi, gi.cpu().numpy())
            hl, hli = a.lattice(grid, want_index=True, dtype=dt)
            gl, gli = b.lattice_dev(grid, want_index=True, dtype=tdt)
            assert np.array_equal(_bits(hl), _bits(gl.cpu().numpy())) and np.array_equal(hli, gli.cpu().numpy())
        q32 = torch.from_numpy(Q.astype(np.float32)).to(dev)
        assert np.array_equal(_bits(a.distance(Q.astype(np.float32))), _bits(b.distance_dev(q32).cpu().numpy()))
        assert b.distance_dev(torch.empty((0, 3), dtype=torch.float64, device=dev)).numel() == 0
        d3 = c.distance(Q)
        b.close()
        pkg._lib.lib().r2s_release_cache()                           # live indices survive it
        again, ai = a.distance(Q, want_index=True)
        assert np.array_equal(_bits(again), _bits(want)) and np.array_equal(ai, wi)
        assert np.array_equal(_bits(c.distance(Q)), _bits(d3))
        with pytest.raises(pkg._lib.R2SError, match="closed"):
            b.info()
        bad = torch.from_numpy(T).to(dev).clone()
        bad[5, 1] = len(V)
        with pytest.raises(pkg._lib.R2SError, match="index"):
            pkg.MeshIndex(torch.from_numpy(V).to(dev), bad)
    finally:
        a.close(), b.close(), c.close()


def _small_gyroid(dtype):
    n = 17
    return R.gyroid(n, 8).astype(dtype).ravel(), n, (-1.0, -1.0, -1.0), 2.0 / (n - 1)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("field", ["sphere", "gyroid"])
def test_redistance_full(pkg, field, dtype):
    if field == "sphere":
        n, origin, h = 17, (-3.0, 1.5, 0.25), 0.25
        f = C.sphere_field(n, 5.2, dtype)
    else:
        f, n, origin, h = _small_gyroid(dtype)
    grid = ((n, n, n), origin, h)
    V, T = _surface(pkg, f, (n, n, n), origin, h)
    out = pkg.redistance_full(f.reshape(n, n, n), grid)
    assert out.dtype == dtype and out.shape == (n, n, n) and len(T) > 200
    P = M.lattice_points((n, n, n), origin, h)
    dr, _ = M.distance_brute(V, T, P)
    L = _scale(V, P)
    frac = np.abs(np.abs(out.ravel().astype(np.float64)) - dr) / M.bound(dr, L, dtype)
    print(f"MESHQ redistance_full {field} {np.dtype(dtype).name}: {len(P)} voxels, {len(T)} triangles, largest fraction of the bound "
          f"{frac.max():.3f} (L = {L:.3f})")
    assert frac.max() <= 1.0
    assert np.array_equal(~np.signbit(out.ravel()), f >= 0.0)         # (_signs of tests/test_redistance_gpu.py)
    import torch
    t = torch.from_numpy(f.reshape(n, n, n)).cuda()
    assert np.array_equal(_bits(pkg.redistance_full_dev(t, grid).cpu().numpy()), _bits(out))
    if field == "sphere":
        ext = pkg.redistance_full(-np.ones((n, n, n), dtype), grid)
        assert ext.dtype == dtype and np.isneginf(ext).all()
        assert np.isposinf(pkg.redistance_full(np.ones((n, n, n), dtype), grid)).all()


def test_surface_deviation_of_shifted_boxes(pkg):
    lo, hi = np.array((-0.75, 0.5, 1.0)), np.array((1.25, 2.0, 1.5))
    s = np.array((0.25, 0.0, 0.0))
    VA, TA = M.box_mesh(lo, hi)
    VB, TB = M.box_mesh(lo + s, hi + s)
    dev = pkg.surface_deviation(VA, TA, VB, TB)
    L = float(max(np.abs(VA).max(), np.abs(VB).max()))
    worst = 0.0
    for key, Vq, blo, bhi in (("a_to_b", VA, lo + s, hi + s), ("b_to_a", VB, lo, hi)):
        want = M.box_distance(Vq.astype(np.float64), blo, bhi)
        b = float(M.bound(want, L, np.float64).max())
        got = dev[key]
        for name, w in (("max", want.max()), ("mean", want.mean()), ("rms", np.sqrt(np.mean(want * want)))):
            worst = max(worst, abs(got[name] - w) / b)
            assert abs(got[name] - w) <= b, (key, name, got[name], w)
        assert abs(want[got["argmax"]] - want.max()) <= b
        assert want.max() == 0.25
    assert abs(dev["hausdorff"] - 0.25) <= M.bound(np.array(0.25), L, np.float64)
    print(f"MESHQ surface_deviation: hausdorff {dev['hausdorff']!r}, largest fraction of the bound {worst:.3f}")


def test_rho2sdf_signed_distance_and_deviation(pkg):
    X, IEN, rho = load_fixture("sphere")
    grid = pkg.Grid(X.min(0), X.max(0), 20, 3)
    opts = pkg.Rho2sdfOptions(threshold_density=0.5, rbf_grid="fine")
    info0 = {}
    plain = pkg.rho2sdf("t", X, IEN, rho, options=opts, sdf_grid=grid, info=info0)
    assert "sdf_distance" not in info0 and "smoothing_deviation" not in info0
    info = {}
    got = pkg.rho2sdf("t", X, IEN, rho, options=opts, sdf_grid=grid, info=info, signed_distance=True, deviation=True)
    assert np.array_equal(_bits(plain[0]), _bits(got[0])) and np.array_equal(_bits(plain[3]), _bits(got[3]))
    assert np.array_equal(plain[1][0], got[1][0]) and plain[1][1:] == got[1][1:] and got[2] is grid
    sd = info["sdf_distance"]
    want = pkg.redistance_full(got[0], grid, 2)
    assert sd.dtype == np.float32 and sd.shape == got[0].shape and np.array_equal(_bits(sd), _bits(want))
    assert np.isfinite(sd).all() and np.array_equal(~np.signbit(sd), got[0] >= 0.0)
    direct = pkg.surface_deviation(*pkg.extract_isosurface(got[0], grid, 2), *pkg.extract_isosurface(got[3], grid, None))
    assert info["smoothing_deviation"] == direct
    assert np.isfinite(direct["hausdorff"]) and direct["hausdorff"] == max(direct["a_to_b"]["max"], direct["b_to_a"]["max"])
    print(f"MESHQ rho2sdf sphere: smoothing moved the surface by at most {direct['hausdorff']:.4g} (cell {grid.cell_size:.4g})")
