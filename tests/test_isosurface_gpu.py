"""Iso-surface extraction on the GPU (r2s_extract_isosurface(_dev), r2s_last_isosurface, r2s_rho2sdf extract_surface):
vertices bit-equal to the numpy restatement of the definition (tests/iso_ref.py), triangles checked without the table
(one cube per triangle, cube order, closed and consistently oriented where the interior stays off the border, Euler
characteristic and volume of a sphere), capacities, determinism, the 513^3 path and the in-call surface."""
import ctypes

import numpy as np
import pytest

import iso_ref as R
from conftest import load_fixture

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a).view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _extract(pkg, values, dims, origin, spacing, iso, caps=None, poison=None):
    """r2s_extract_isosurface -> (nv, nt, verts, tris) with room for caps = (vcap, tcap) entries (None: the full counts)"""
    L = pkg._lib
    a = np.ascontiguousarray(values)
    d = (ctypes.c_int64 * 3)(*dims)
    o = (ctypes.c_double * 3)(*origin)
    nv, nt = ctypes.c_int64(-1), ctypes.c_int64(-1)
    f32 = int(a.dtype == np.float32)
    if caps is None:
        L.check(L.lib().r2s_extract_isosurface(a.ctypes.data_as(ctypes.c_void_p), f32, d, o, spacing, iso, -1, None, 0, None, 0,
                                               ctypes.byref(nv), ctypes.byref(nt)))
        caps = (nv.value, nt.value)
    v = np.full((caps[0] + 2, 3), poison if poison is not None else 0, np.float32)
    t = np.full((caps[1] + 2, 3), -7, np.int32)
    L.check(L.lib().r2s_extract_isosurface(a.ctypes.data_as(ctypes.c_void_p), f32, d, o, spacing, iso, -1,
                                           v.ctypes.data_as(L.c_float_p), caps[0], t.ctypes.data_as(L.c_int32_p), caps[1],
                                           ctypes.byref(nv), ctypes.byref(nt)))
    return nv.value, nt.value, v, t


def _mesh(pkg, values, dims, origin=(0.0, 0.0, 0.0), spacing=1.0, iso=0.0):
    nv, nt, v, t = _extract(pkg, values, dims, origin, spacing, iso)
    assert (t[nt:] == -7).all()
    return v[:nv], t[:nt]


def _check_vertices(pkg, values, dims, origin, spacing, iso, label):
    verts, tris = _mesh(pkg, values, dims, origin, spacing, iso)
    want, keys = R.vertices(values, dims, origin, spacing, iso)
    assert verts.shape == want.shape, (label, verts.shape, want.shape)
    assert np.array_equal(_bits(verts), _bits(want)), f"{label}: {int((_bits(verts) != _bits(want)).any(1).sum())} vertices differ"
    assert tris.size == 0 or (tris.min() >= 0 and tris.max() < len(verts))
    if len(tris):
        R.check_cube_locality(keys, tris, dims)
    return verts, tris, keys


def _sphere(n, r, dtype):
    g = np.arange(n, dtype=np.float64) - (n - 1) / 2
    z, y, x = np.meshgrid(g, g, g, indexing="ij")
    return (r - np.sqrt(x * x + y * y + z * z)).astype(dtype).ravel()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_sphere(pkg, dtype):
    n, r, h = 48, 16.0, 0.25
    origin = (-3.0, 1.5, 0.25)
    verts, tris, keys = _check_vertices(pkg, _sphere(n, r, dtype), (n, n, n), origin, h, 0.0, f"sphere {dtype.__name__}")
    dup, unpaired = R.unpaired_edges(tris, len(verts))
    assert len(dup) == 0 and len(unpaired) == 0, "not a closed, consistently oriented 2-manifold"
    assert R.euler(tris, len(verts)) == 2
    vol = R.signed_volume(verts, tris)
    exact = 4.0 / 3.0 * np.pi * (r * h) ** 3
    assert vol > 0 and abs(vol / exact - 1) < 0.015, vol / exact


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_odd_dims_origin_spacing_iso(pkg, dtype):
    nx, ny, nz = 37, 23, 41
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    f = np.sin(0.31 * i + 0.2) * np.cos(0.27 * j) + 0.8 * np.sin(0.19 * k - 0.4) + 0.05 * np.cos(0.9 * i * j / nx)
    f = f.astype(dtype).ravel()
    verts, tris, keys = _check_vertices(pkg, f, (nx, ny, nz), (-1.25, 0.5, 3.0), 0.037, 0.3, "odd dims")
    assert len(verts) > 1000
    dup, unpaired = R.unpaired_edges(tris, len(verts))
    assert len(dup) == 0
    assert R.on_boundary_face(keys, unpaired, len(verts), (nx, ny, nz)).all(), "an open edge inside the lattice"


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_noise_with_exact_iso_nan_and_inf(pkg, dtype, seed):
    rng = np.random.default_rng(seed)
    n = 12
    f = rng.normal(size=(n, n, n))
    f[rng.random(f.shape) < 0.2] = 0.25                 # exactly iso
    f[rng.random(f.shape) < 0.05] = np.nan
    f[rng.random(f.shape) < 0.05] = np.inf
    f[rng.random(f.shape) < 0.05] = -np.inf
    f[0], f[-1], f[:, 0], f[:, -1], f[:, :, 0], f[:, :, -1] = (-1.0,) * 6
    f = f.astype(dtype).ravel()
    verts, tris, keys = _check_vertices(pkg, f, (n, n, n), (0.5, -0.5, 2.0), 0.5, 0.25, f"noise {seed}")
    dup, unpaired = R.unpaired_edges(tris, len(verts))
    assert len(dup) == 0 and len(unpaired) == 0


def test_border_touching_interior(pkg):
    n = 30
    g = np.arange(n, dtype=np.float64)
    z, y, x = np.meshgrid(g, g, g, indexing="ij")
    f = (9.0 - np.sqrt((x - 2) ** 2 + (y - 15) ** 2 + (z - 27) ** 2)).ravel()
    verts, tris, keys = _check_vertices(pkg, f, (n, n, n), (0.0, 0.0, 0.0), 1.0, 0.0, "border")
    dup, unpaired = R.unpaired_edges(tris, len(verts))
    assert len(dup) == 0 and len(unpaired) > 0
    assert R.on_boundary_face(keys, unpaired, len(verts), (n, n, n)).all()


def test_empty(pkg):
    dims = (9, 7, 5)
    for f in (-np.ones(315), np.ones(315), np.full(315, np.nan)):
        verts, tris = _mesh(pkg, f, dims)
        assert verts.shape == (0, 3) and tris.shape == (0, 3)
    grid = pkg.Grid(np.zeros(3), np.ones(3), 6, 1)
    v, t = pkg.extract_isosurface(-np.ones(grid.ngp, np.float32), grid)
    assert v.shape == (0, 3) and t.shape == (0, 3) and v.dtype == np.float32 and t.dtype == np.int32


def test_capacities(pkg):
    f, dims = _sphere(24, 7.0, np.float32), (24, 24, 24)
    nv, nt, v, t = _extract(pkg, f, dims, (0, 0, 0), 1.0, 0.0)
    nv0, nt0, _, _ = _extract(pkg, f, dims, (0, 0, 0), 1.0, 0.0, caps=(0, 0))
    assert (nv0, nt0) == (nv, nt) and nv > 100
    for cv, ct in ((nv // 3, nt // 2), (nv, 5), (7, nt)):
        m, k, pv, pt = _extract(pkg, f, dims, (0, 0, 0), 1.0, 0.0, caps=(cv, ct), poison=np.float32(-123.5))
        assert (m, k) == (nv, nt)
        assert np.array_equal(_bits(pv[:cv]), _bits(v[:cv])) and (pv[cv:] == np.float32(-123.5)).all()
        assert np.array_equal(pt[:ct], t[:ct]) and (pt[ct:] == -7).all()


def test_deterministic_and_device_variant(pkg):
    import torch
    grid = pkg.Grid(np.array([0.1, -0.2, 0.3]), np.array([2.1, 1.1, 1.4]), 60, 2)
    nx, ny, nz = grid.dims
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    f = (np.sin(0.2 * i) + np.cos(0.23 * j) * np.sin(0.17 * k + 0.3)).astype(np.float32)
    a = pkg.extract_isosurface(f, grid, iso=0.1)
    b = pkg.extract_isosurface(f, grid, iso=0.1)
    assert len(a[0]) > 1000
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(a[1], b[1])
    dv, dt = pkg.extract_isosurface_dev(torch.from_numpy(f).to("cuda:0"), grid, iso=0.1)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(dv.cpu().numpy()), _bits(a[0])) and np.array_equal(dt.cpu().numpy(), a[1])
    d64 = pkg.extract_isosurface_dev(torch.from_numpy(f.astype(np.float64)).to("cuda:0"), grid, iso=0.1)
    h64 = pkg.extract_isosurface(f.astype(np.float64), grid, iso=0.1)
    assert np.array_equal(_bits(d64[0].cpu().numpy()), _bits(h64[0])) and np.array_equal(d64[1].cpu().numpy(), h64[1])
    want, _ = R.vertices(f, grid.dims, grid.AABB_min, grid.cell_size, 0.1)
    assert np.array_equal(_bits(a[0]), _bits(want))


def test_large_gyroid(pkg):
    n = 513
    f = R.gyroid(n, 24)
    verts, tris = _mesh(pkg, f, (n, n, n), (-1.0, -1.0, -1.0), 2.0 / (n - 1), 0.0)
    assert len(verts) > (1 << 24)
    want, keys = R.vertices(f, (n, n, n), (-1.0, -1.0, -1.0), 2.0 / (n - 1), 0.0)
    assert np.array_equal(_bits(verts), _bits(want))
    del want
    assert tris.min() >= 0 and tris.max() < len(verts)
    sel = np.random.default_rng(4).choice(len(tris), 1 << 20, replace=False)
    sel.sort()
    R.check_cube_locality(keys, tris[sel], (n, n, n))


def _beam_cases(pkg):
    X, IEN, rho = load_fixture("beam_vfrac_03")
    auto = pkg.noninteractive_sdf_grid_setup(pkg.Mesh(X, IEN))
    yield "same", (X, IEN, rho), dict(sdf_grid_setup="automatic", rbf_grid="same"), auto
    yield "fine", (X, IEN, rho), dict(sdf_grid_setup="automatic", rbf_grid="fine"), auto
    X4, IEN4, rho4 = load_fixture("beam_vfrac_04")
    yield "early", (X4, IEN4, rho4), dict(threshold_density=0.518555, rbf_grid="fine"), pkg.Grid(X4.min(0), X4.max(0), 250, 3)


def test_rho2sdf_surface(pkg, tmp_path):
    for name, (X, IEN, rho), kw, grid in _beam_cases(pkg):
        smooth = 2 if kw["rbf_grid"] == "fine" else 1
        nfine = int(np.prod([int(n) * smooth + 1 for n in grid.N]))
        if name == "early":
            assert nfine >= (1 << 22) and nfine >= 162 ** 3
        opts = pkg.Rho2sdfOptions(**kw)
        off = pkg.rho2sdf("t", X, IEN, rho, options=opts, sdf_grid=grid, info={})
        for pinned in (True, False):
            info = {}
            on = pkg.rho2sdf("t", X, IEN, rho, options=opts, sdf_grid=grid, info=info, surface=True, pinned_results=pinned)
            verts, tris = info["surface"]
            assert len(tris) > 100, name
            want = pkg.extract_isosurface(on[0], grid, smooth)
            assert np.array_equal(_bits(verts), _bits(want[0])) and np.array_equal(tris, want[1]), (name, pinned)
            assert np.array_equal(_bits(on[0]), _bits(off[0])) and np.array_equal(_bits(on[3]), _bits(off[3])), (name, pinned)
            assert on[1][1] == off[1][1] and on[1][2] == off[1][2]
    X, IEN, rho = load_fixture("beam_vfrac_03")
    o = pkg._lib.R2SOptions()
    pkg._lib.lib().r2s_default_options(ctypes.byref(o))
    o.skip_rbf = 1
    o.extract_surface = 1
    mesh = pkg.Mesh(X, IEN)
    grid = pkg.noninteractive_sdf_grid_setup(mesh)
    rc = pkg._lib.lib().r2s_rho2sdf(mesh.X.ctypes.data_as(pkg._lib.c_double_p), mesh.nnp, mesh.IEN.ctypes.data_as(pkg._lib.c_int64_p),
                                    mesh.nel, np.ascontiguousarray(rho).ctypes.data_as(pkg._lib.c_double_p), ctypes.byref(o),
                                    ctypes.byref(grid.c), None, None, None, None, None)
    assert rc == -1


def test_stl_of_a_gpu_mesh(pkg, tmp_path):
    verts, tris = _mesh(pkg, _sphere(20, 6.0, np.float32), (20, 20, 20), (1.0, 2.0, 3.0), 0.5, 0.0)
    path = pkg.export_stl(str(tmp_path / "sphere"), verts, tris)
    with open(path, "rb") as fh:
        data = fh.read()
    assert not data[:80].startswith(b"solid") and int(np.frombuffer(data[80:84], "<u4")[0]) == len(tris)
    rec = np.frombuffer(data[84:], dtype=np.dtype([("n", "<f4", 3), ("v", "<f4", (3, 3)), ("attr", "<u2")]))
    assert np.array_equal(rec["v"], verts[tris])
    c = verts[tris].mean(axis=1) - np.array([1.0, 2.0, 3.0]) - 0.5 * 9.5
    assert (np.einsum("ij,ij->i", rec["n"], c) > 0).mean() > 0.99      # normals point outwards
