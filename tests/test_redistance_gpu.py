"""Redistancing on the GPU (r2s_mesh_distance(_dev), r2s_redistance(_dev), rho2sdf(redistance_cells=...)) against the float64
restatement of the header's definition (tests/mesh_dist_ref64.py).  Every voxel is compared:

    |out - min(d_ref, band)| <= u |ref| + K 2^-52 L        u = 2^-24 (Float32 output) or 2^-53, K and L as in the helper.

min(d, band) is 1-Lipschitz, so a voxel within the bound of `band` may come out clamped or not; for those voxels alone the
index may be -1 or a triangle.  Everywhere else the reference distance to the reported triangle is within the bound of d_ref
and -1 appears exactly where the output is `band`.  Each test prints the largest fraction of the bound used ("REDIST ...").
Largest fraction observed on an MI355X: see DESIGN.md "Redistancing"."""
import ctypes
import functools
import os

import numpy as np
import pytest

import iso_ref as R
import mesh_dist_ref64 as M
from conftest import load_fixture

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a).view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _lat(dims, origin):
    return (ctypes.c_int64 * 3)(*dims), (ctypes.c_double * 3)(*origin)


def _surface(pkg, f, dims, origin, h, iso):
    L = pkg._lib
    a = np.ascontiguousarray(f)
    d, o = _lat(dims, origin)
    nv, nt = ctypes.c_int64(), ctypes.c_int64()
    L.check(L.lib().r2s_extract_isosurface(a.ctypes.data_as(ctypes.c_void_p), int(a.dtype == np.float32), d, o, h, iso, -1, None, 0,
                                           None, 0, ctypes.byref(nv), ctypes.byref(nt)))
    V, T = np.empty((nv.value, 3), np.float32), np.empty((nt.value, 3), np.int32)
    L.check(L.lib().r2s_last_isosurface(V.ctypes.data_as(L.c_float_p), nv.value, T.ctypes.data_as(L.c_int32_p), nt.value,
                                        ctypes.byref(nv), ctypes.byref(nt)))
    return V, T


def _redist(pkg, f, dims, origin, h, iso, band):
    L = pkg._lib
    a = np.ascontiguousarray(f)
    out = np.full(a.shape, 777.0, a.dtype)
    d, o = _lat(dims, origin)
    L.check(L.lib().r2s_redistance(a.ctypes.data_as(ctypes.c_void_p), int(a.dtype == np.float32), d, o, h, iso, band, -1,
                                   out.ctypes.data_as(ctypes.c_void_p)))
    return out


def _mesh_dist(pkg, V, T, dims, origin, h, band, dtype=np.float64, index=True, rc=False):
    L = pkg._lib
    V, T = np.ascontiguousarray(V, np.float32), np.ascontiguousarray(T, np.int32)
    n = int(np.prod(dims))
    out, idx = np.full(n, 777.0, dtype), np.full(n, -9, np.int32)
    d, o = _lat(dims, origin)
    code = L.lib().r2s_mesh_distance(V.ctypes.data_as(L.c_float_p), len(V), T.ctypes.data_as(L.c_int32_p), len(T), d, o, h, band,
                                     int(dtype == np.float32), -1, out.ctypes.data_as(ctypes.c_void_p),
                                     idx.ctypes.data_as(L.c_int32_p) if index else None)
    if rc:
        return code, out, idx
    L.check(code)
    return out, idx


def _compare(label, out, idx, V, T, dims, origin, h, band, ref=None):
    """the bound on every voxel and the index rule; `out` unsigned or signed (|out| is compared) -> the reference tuple"""
    ref = ref or M.lattice_distance(V, T, dims, origin, h, band)
    d, ridx, raw, _ = ref
    L = M.coord_scale(V, dims, origin, h)
    mag = np.abs(out.astype(np.float64)).ravel()
    assert np.isfinite(mag).all(), label
    b = M.bound(d, L, out.dtype)
    frac = np.abs(mag - d) / b
    print(f"REDIST {label}: {len(d)} voxels, {len(T)} triangles, {(ridx >= 0).sum()} in band, largest fraction of the bound "
          f"{frac.max():.3f} (L = {L:.3f})")
    assert frac.max() <= 1.0, (label, int((frac > 1).sum()), frac.max())
    if idx is not None:
        idx = idx.ravel()
        near = np.abs(raw - band) <= b                     # may come out clamped or not
        assert ((idx >= -1) & (idx < max(len(T), 1))).all()
        strict = ~near
        assert np.array_equal((idx == -1)[strict], (mag == np.dtype(out.dtype).type(band))[strict]), label
        assert np.array_equal((idx == -1)[strict], (ridx == -1)[strict]), label
        has = idx >= 0
        if has.any():
            P = M.lattice_points(dims, origin, h)[has]
            dt = M.distance_to_given(V, T, P, idx[has])
            ok = np.abs(dt - raw[has]) <= M.bound(raw[has], L, np.float64)
            assert ok.all(), (label, "the reported triangle is not a closest one", int((~ok).sum()))
    return ref


def _signs(label, out, f, iso):
    inside = np.asarray(f).ravel() >= iso
    assert np.array_equal(~np.signbit(out.ravel()), inside), label


def _sphere(n, r, dtype, center=None):
    g = np.arange(n, dtype=np.float64)
    c = (n - 1) / 2 if center is None else None
    cz, cy, cx = (c, c, c) if center is None else center[::-1]
    z, y, x = np.meshgrid(g, g, g, indexing="ij")
    return (r - np.sqrt((x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2)).astype(dtype).ravel()


def _signed_case(pkg, label, f, dims, origin, h, iso, band):
    V, T = _surface(pkg, f, dims, origin, h, iso)
    out = _redist(pkg, f, dims, origin, h, iso, band)
    assert out.dtype == f.dtype
    ref = _compare(label, out, None, V, T, dims, origin, h, band)
    _signs(label, out, f, iso)
    return out, V, T, ref


# ---- redistance on extracted surfaces ----------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_sphere(pkg, dtype):
    n, h = 24, 0.25
    f = _sphere(n, 9.0, dtype)
    out, V, T, _ = _signed_case(pkg, f"sphere {dtype.__name__}", f, (n, n, n), (-3.0, 1.5, 0.25), h, 0.0, 3.5 * h)
    assert len(T) > 1000 and (np.abs(out) < 3.5 * h).sum() > 1000


@functools.lru_cache(maxsize=None)
def _gyroid_case(n, period):
    return R.gyroid(n, period).ravel(), (n, n, n), (-1.0, -1.0, -1.0), 2.0 / (n - 1)


_shared = {}


def _gyroid13(pkg):
    """case 2, shared with the order-independence test: (f, lattice, band, out, V, T, ref)"""
    if "g13" not in _shared:
        f, dims, origin, h = _gyroid_case(40, 13)
        band = 2.5 * h
        out, V, T, ref = _signed_case(pkg, "gyroid 40^3 period 13", f, dims, origin, h, 0.0, band)
        _shared["g13"] = (f, dims, origin, h, band, out, V, T, ref)
    return _shared["g13"]


def test_gyroid_several_sheets(pkg):
    f, dims, origin, h, band, out, V, T, ref = _gyroid13(pkg)
    assert len(T) > 10000


def test_gyroid_long_lists_and_batches(pkg):
    f, dims, origin, h = _gyroid_case(40, 5)
    band = 3.0 * h
    out, V, T, _ = _signed_case(pkg, "gyroid 40^3 period 5", f, dims, origin, h, 0.0, band)
    st = pkg.last_distance_stats()
    assert st["pairs"] / max(st["n_active_tiles"], 1) > 1000, "tile lists of thousands of triangles (more than one LDS chunk)"
    assert st["batches"] == 1
    os.environ["R2S_REDIST_WORKSPACE_MB"] = "0.001"
    try:
        again = _redist(pkg, f, dims, origin, h, 0.0, band)
        st = pkg.last_distance_stats()
    finally:
        del os.environ["R2S_REDIST_WORKSPACE_MB"]
    assert st["batches"] >= 4, st
    assert np.array_equal(_bits(again), _bits(out)), "the batched run differs from the unbatched one"


def test_band_wider_than_the_grid(pkg):
    n, h = 20, 0.5
    f = _sphere(n, 6.0, np.float64)
    out, V, T, ref = _signed_case(pkg, "band 100 cells", f, (n, n, n), (0.3, -0.2, 0.1), h, 0.0, 100 * h)
    assert (np.abs(out) < 100 * h).all() and (ref[1] >= 0).all()


def test_narrow_band(pkg):
    n, h = 24, 0.25
    f = _sphere(n, 9.0, np.float32)
    out, V, T, _ = _signed_case(pkg, "band 0.3 cell", f, (n, n, n), (-3.0, 1.5, 0.25), h, 0.0, 0.3 * h)
    clamped = np.abs(out) == np.float32(0.3 * h)
    assert 0.8 < clamped.mean() < 1.0


def test_plane_through_lattice_points(pkg):
    """f = x - 5 with integer values: exact-iso lattice points, degenerate triangles, unwelded coincident vertices"""
    dims, origin, h = (12, 9, 7), (0.5, -0.25, 2.0), 0.5
    k, j, i = np.meshgrid(np.arange(7.0), np.arange(9.0), np.arange(12.0), indexing="ij")
    f = (i - 5.0).ravel()
    out, V, T, _ = _signed_case(pkg, "plane x = 5", f, dims, origin, h, 0.0, 3.0 * h)
    assert np.isfinite(out).all()
    o3 = out.reshape(7, 9, 12)
    assert (o3[:, :, 5] == 0.0).all()
    assert np.array_equal(~np.signbit(out), f >= 0.0)


def test_empty_surfaces(pkg):
    dims, h, band = (9, 7, 5), 0.5, 1.25
    for f, sign in ((-np.ones(315), -1.0), (np.ones(315), 1.0), (np.full(315, np.nan), -1.0), (np.ones(315, np.float32), 1.0)):
        out = _redist(pkg, f, dims, (0.0, 0.0, 0.0), h, 0.0, band)
        assert (out == f.dtype.type(sign * band)).all()
    # NaN voxels inside a sphere count as exterior: a surface around them, negative sign on them
    n = 16
    f = _sphere(n, 5.0, np.float64)
    f3 = f.reshape(n, n, n)
    f3[7:9, 7:9, 7:9] = np.nan
    out, V, T, _ = _signed_case(pkg, "NaN voxels", f, (n, n, n), (0.0, 0.0, 0.0), 1.0, 0.0, 2.5)
    assert (out.reshape(n, n, n)[7:9, 7:9, 7:9] < 0).all()
    d, idx = _mesh_dist(pkg, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), dims, (0.0, 0.0, 0.0), h, band)
    assert (d == band).all() and (idx == -1).all()


@pytest.mark.parametrize("dims", [(17, 9, 33), (2, 2, 2)])
def test_border_dims(pkg, dims):
    nx, ny, nz = dims
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    f = (np.sin(0.45 * i + 0.2) * np.cos(0.4 * j) + 0.8 * np.sin(0.3 * k - 0.4) + 0.1).astype(np.float32).ravel()
    _signed_case(pkg, f"dims {dims}", f, dims, (-1.25, 0.5, 3.0), 0.37, 0.0, 2.5 * 0.37)


def test_sphere_touching_the_border(pkg):
    n = 30
    f = _sphere(n, 9.0, np.float64, center=(2.0, 15.0, 27.0))
    out, V, T, _ = _signed_case(pkg, "open mesh", f, (n, n, n), (0.0, 0.0, 0.0), 1.0, 0.0, 3.0)
    dup, unpaired = R.unpaired_edges(T, len(V))
    assert len(unpaired) > 0


def test_gyroid_129_sampled(pkg):
    """the index and offset path at size: 4096 random voxels against candidates from a k-d tree over the centroids"""
    from scipy.spatial import cKDTree
    n = 129
    f, dims, origin, h = _gyroid_case(n, 24)
    band = 4.0 * h
    V, T = _surface(pkg, f, dims, origin, h, 0.0)
    out = _redist(pkg, f, dims, origin, h, 0.0, band)
    _signs("gyroid 129", out, f, 0.0)
    L = M.coord_scale(V, dims, origin, h)
    rng = np.random.default_rng(7)
    pick = rng.choice(n ** 3, 4096, replace=False)
    ax = M.lattice_axes(dims, origin, h)
    P = np.stack([ax[0][pick % n], ax[1][(pick // n) % n], ax[2][pick // (n * n)]], axis=1)
    mag = np.abs(out[pick].astype(np.float64))
    Vd = V.astype(np.float64)
    tri = Vd[T]
    longest = np.sqrt(max(((tri[:, a] - tri[:, b]) ** 2).sum(axis=1).max() for a, b in ((0, 1), (0, 2), (1, 2))))
    slack = M.bound(mag, L, out.dtype)
    cand = cKDTree(tri.mean(axis=1)).query_ball_point(P, mag + longest + slack)
    counts = np.array([len(c) for c in cand])
    assert (counts[mag < np.float32(band)] > 0).all()
    flat = np.concatenate([np.asarray(c, np.int64) for c in cand])
    owner = np.repeat(np.arange(len(P)), counts)
    dd = M.distance_to_given(V, T, P[owner], flat)
    ref = np.full(len(P), np.inf)
    np.minimum.at(ref, owner, dd)
    ref = np.minimum(ref, band)
    frac = np.abs(mag - ref) / M.bound(ref, L, out.dtype)
    print(f"REDIST gyroid 129^3 period 24: 4096 sampled voxels, {len(T)} triangles, {int((ref < band).sum())} in band, "
          f"largest fraction of the bound {frac.max():.3f} (L = {L:.3f})")
    assert frac.max() <= 1.0


# ---- r2s_mesh_distance on arbitrary meshes -----------------------------------------------------------------------------

def test_box_spanning_many_tiles(pkg):
    dims, origin, h = (33, 33, 33), (0.1, -0.3, 0.7), 0.3
    lo, hi = (1.3, 0.9, 2.1), (8.5, 7.7, 9.3)
    V, T = M.box_mesh(lo, hi)
    band = 2.0
    for dtype in (np.float64, np.float32):
        d, idx = _mesh_dist(pkg, V, T, dims, origin, h, band, dtype)
        _compare(f"box {np.dtype(dtype).name}", d, idx, V, T, dims, origin, h, band)
        P = M.lattice_points(dims, origin, h)
        want = np.minimum(M.box_distance(P, V.astype(np.float64).min(0), V.astype(np.float64).max(0)), band)
        L = M.coord_scale(V, dims, origin, h)
        assert (np.abs(d.astype(np.float64) - want) <= M.bound(want, L, dtype)).all()


def test_order_independence(pkg):
    f, dims, origin, h, band, out, V, T, ref = _gyroid13(pkg)
    d1, i1 = _mesh_dist(pkg, V, T, dims, origin, h, band, np.float32)
    assert np.array_equal(_bits(np.abs(out)), _bits(d1)), "redistance and mesh_distance differ on the same mesh"
    _compare("gyroid 13 index", d1, i1, V, T, dims, origin, h, band, ref=ref)
    perm = np.random.default_rng(1).permutation(len(T))
    d2, i2 = _mesh_dist(pkg, V, T[perm], dims, origin, h, band, np.float32)
    assert np.array_equal(_bits(d1), _bits(d2)), "the distances depend on the order of the triangles"
    _, ridx, raw, second = ref
    L = M.coord_scale(V, dims, origin, h)
    unique = (ridx >= 0) & (second - raw > 2 * M.bound(raw, L, np.float64)) & (raw < band - M.bound(raw, L, np.float32))
    assert unique.sum() > 1000
    assert np.array_equal(perm[i2[unique]], i1[unique]) and np.array_equal(i1[unique], ridx[unique])


def test_host_and_dev_variants(pkg):
    import torch
    f, dims, origin, h, band, out, V, T, ref = _gyroid13(pkg)
    lattice = (dims, origin, h)
    d64, i64 = _mesh_dist(pkg, V, T, dims, origin, h, band, np.float64)
    d32, _ = _mesh_dist(pkg, V, T, dims, origin, h, band, np.float32, index=False)   # closest_tri_out = NULL
    assert np.array_equal(_bits(d64.astype(np.float32)), _bits(d32)), "Float32 is not the one rounding of Float64"
    tv, tt = torch.from_numpy(V).cuda(), torch.from_numpy(T).cuda()
    g64, gi = pkg.mesh_distance_dev(tv, tt, lattice, band, want_index=True)
    g32 = pkg.mesh_distance_dev(tv, tt, lattice, band, dtype=torch.float32)
    assert np.array_equal(_bits(g64.cpu().numpy().ravel()), _bits(d64)) and np.array_equal(gi.cpu().numpy().ravel(), i64)
    assert np.array_equal(_bits(g32.cpu().numpy().ravel()), _bits(d32))
    a, ai = pkg.mesh_distance(V, T, lattice, band, want_index=True)
    assert np.array_equal(_bits(a.ravel()), _bits(d64)) and np.array_equal(ai.ravel(), i64) and a.shape == dims[::-1]
    # redistance: host and device variants
    grid = pkg.Grid([0.0, 0.0, 0.0], [1.0, 1.0, 1.0], 10, 3)
    n = grid.dims
    fs = _sphere(n[0], 4.0, np.float32).reshape(n[::-1])
    r_host = pkg.redistance(fs, grid, band=2.5 * grid.cell_size)
    r_dev = pkg.redistance_dev(torch.from_numpy(fs).cuda(), grid, band=2.5 * grid.cell_size)
    assert r_host.shape == fs.shape and np.array_equal(_bits(r_host), _bits(r_dev.cpu().numpy()))
    Vs, Ts = pkg.extract_isosurface(fs, grid)
    _compare("api sphere", r_host.ravel(), None, Vs, Ts, n, tuple(grid.AABB_min), grid.cell_size, 2.5 * grid.cell_size)
    pkg._lib.lib().r2s_release_cache()
    assert np.array_equal(_bits(pkg.redistance(fs, grid, band=2.5 * grid.cell_size)), _bits(r_host))


def test_refusals(pkg):
    import torch
    V, T = M.box_mesh((0.2, 0.2, 0.2), (1.4, 1.4, 1.4))
    good = dict(dims=(6, 6, 6), origin=(0.0, 0.0, 0.0), h=0.3, band=1.0)
    ARG = -1
    for kw in (dict(dims=(6, 1, 6)), dict(h=0.0), dict(h=-1.0), dict(h=np.nan), dict(h=np.inf), dict(band=0.0), dict(band=-2.0),
               dict(band=np.inf), dict(band=np.nan), dict(origin=(0.0, np.inf, 0.0))):
        a = dict(good)
        a.update(kw)
        rc, out, idx = _mesh_dist(pkg, V, T, a["dims"], a["origin"], a["h"], a["band"], rc=True)
        assert rc == ARG and (out == 777.0).all() and (idx == -9).all(), kw
    Tb = T.copy()
    Tb[5, 2] = len(V)                                                # == n_verts
    Vb = V.copy()
    Vb[2, 1] = np.nan
    for v, t in ((V, Tb), (Vb, T)):
        rc, out, idx = _mesh_dist(pkg, v, t, good["dims"], good["origin"], good["h"], good["band"], rc=True)
        assert rc == ARG and (out == 777.0).all() and (idx == -9).all()
        # the _dev variant decides with its check kernel, before any kernel that follows an index
        out_t = torch.full((6, 6, 6), 777.0, dtype=torch.float64, device="cuda")
        d, o = _lat(good["dims"], good["origin"])
        tv, tt = torch.from_numpy(v).cuda(), torch.from_numpy(t).cuda()
        L = pkg._lib
        rc = L.lib().r2s_mesh_distance_dev(ctypes.c_void_p(tv.data_ptr()), len(v), ctypes.c_void_p(tt.data_ptr()), len(t), d, o,
                                           good["h"], good["band"], 0, ctypes.c_void_p(out_t.data_ptr()), None,
                                           ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == ARG and bool((out_t == 777.0).all())
    f = np.zeros(216)
    L = pkg._lib
    d, o = _lat(good["dims"], good["origin"])
    out = np.full(216, 777.0)
    for iso, h, band, dd in ((np.nan, 0.3, 1.0, d), (0.0, 0.0, 1.0, d), (0.0, 0.3, np.nan, d), (0.0, 0.3, 1.0, (ctypes.c_int64 * 3)(6, 6, 1))):
        rc = L.lib().r2s_redistance(f.ctypes.data_as(ctypes.c_void_p), 0, dd, o, h, iso, band, -1, out.ctypes.data_as(ctypes.c_void_p))
        assert rc == ARG and (out == 777.0).all()


# ---- Python layer ------------------------------------------------------------------------------------------------------

def test_rho2sdf_redistance_cells(pkg):
    X, IEN, rho = load_fixture("sphere")
    grid = pkg.Grid(X.min(0), X.max(0), 20, 3)
    opts = pkg.Rho2sdfOptions(threshold_density=0.5, rbf_grid="fine")
    info0 = {}
    plain = pkg.rho2sdf("t", X, IEN, rho, options=opts, sdf_grid=grid, info=info0)
    assert "sdf_redistanced" not in info0
    info = {}
    got = pkg.rho2sdf("t", X, IEN, rho, options=opts, sdf_grid=grid, redistance_cells=3, info=info)
    assert np.array_equal(_bits(plain[0]), _bits(got[0])) and np.array_equal(_bits(plain[3]), _bits(got[3]))
    assert np.array_equal(plain[1][0], got[1][0]) and plain[1][1:] == got[1][1:] and got[2] is grid
    sd = info["sdf_redistanced"]
    spacing = grid.cell_size / 2
    want = pkg.redistance(got[0], grid, 2, band=3 * spacing)
    assert sd.dtype == np.float32 and sd.shape == got[0].shape and np.array_equal(_bits(sd), _bits(want))
    # Eikonal sanity (not the pin): |grad| by central differences where the stencil stays inside the band
    s = sd.astype(np.float64)
    gz, gy, gx = np.gradient(s, spacing)
    core = np.zeros(s.shape, bool)
    core[1:-1, 1:-1, 1:-1] = True
    sel = core & (np.abs(s) < 3 * spacing - 2 * spacing)
    norm = np.sqrt(gx ** 2 + gy ** 2 + gz ** 2)[sel]
    print(f"REDIST rho2sdf sphere: {int(sel.sum())} voxels with |d| < band - 2 cells, median |grad| {np.median(norm):.4f}")
    assert sel.sum() > 500 and abs(np.median(norm) - 1.0) < 0.02
