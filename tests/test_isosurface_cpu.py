"""Host-side parts of the iso-surface feature (no GPU): the binary STL writer, the argument errors that come before any
device work, and the no-device error of the extraction."""
import ctypes
import os

import numpy as np
import pytest


def _read_stl(path):
    with open(path, "rb") as fh:
        data = fh.read()
    header, count = data[:80], int(np.frombuffer(data[80:84], "<u4")[0])
    rec = np.frombuffer(data[84:], dtype=np.dtype([("n", "<f4", 3), ("v", "<f4", (3, 3)), ("attr", "<u2")]))
    return header, count, rec, len(data)


def test_stl_round_trip(pkg, tmp_path):
    verts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [2, 0, 0]], np.float32)
    tris = np.array([[0, 1, 2], [0, 3, 1], [0, 1, 4]], np.int32)   # the last one has zero area
    path = pkg.export_stl(str(tmp_path / "mesh"), verts, tris)
    assert path.endswith("mesh.stl") and os.path.exists(path)
    header, count, rec, size = _read_stl(path)
    assert not header.lower().startswith(b"solid")
    assert count == 3 and size == 84 + 50 * 3
    assert np.array_equal(rec["v"], verts[tris])
    assert (rec["attr"] == 0).all()
    assert np.array_equal(rec["n"][0], [0, 0, 1]) and np.array_equal(rec["n"][1], [0, 1, 0])
    assert np.array_equal(rec["n"][2], [0, 0, 0])
    # normals: float32 normalised (v1-v0) x (v2-v0)
    rng = np.random.default_rng(3)
    v = rng.normal(size=(40, 3)).astype(np.float32)
    t = rng.integers(0, 40, size=(60, 3)).astype(np.int32)
    path = pkg.export_stl(str(tmp_path / "random.stl"), v, t)
    assert path.endswith("random.stl") and not os.path.exists(path + ".stl")
    _, count, rec, _ = _read_stl(path)
    n = np.cross(v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]])
    ln = np.linalg.norm(n, axis=1, keepdims=True)
    want = np.where(ln > 0, n / np.where(ln > 0, ln, 1), 0)
    assert count == 60 and np.allclose(rec["n"], want, atol=1e-6) and np.array_equal(rec["v"], v[t])
    path = pkg.export_stl(str(tmp_path / "empty"), np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    _, count, rec, size = _read_stl(path)
    assert count == 0 and len(rec) == 0 and size == 84
    with pytest.raises(pkg._lib.R2SError, match="outside"):
        pkg.export_stl(str(tmp_path / "bad"), verts, np.array([[0, 1, 5]], np.int32))


def _call(pkg, dims=(4, 4, 4), spacing=1.0, iso=0.0, caps=(0, 0), dev=False):
    L = pkg._lib
    lib = L.lib()
    values = np.zeros(int(np.prod(dims)) if min(dims) > 0 else 1, np.float32)
    d = (ctypes.c_int64 * 3)(*dims)
    o = (ctypes.c_double * 3)(0.0, 0.0, 0.0)
    nv, nt = ctypes.c_int64(-1), ctypes.c_int64(-1)
    if dev:
        return lib.r2s_extract_isosurface_dev(values.ctypes.data_as(ctypes.c_void_p), 1, d, o, spacing, iso, None, caps[0], None,
                                              caps[1], ctypes.byref(nv), ctypes.byref(nt), None)
    return lib.r2s_extract_isosurface(values.ctypes.data_as(ctypes.c_void_p), 1, d, o, spacing, iso, -1, None, caps[0], None,
                                      caps[1], ctypes.byref(nv), ctypes.byref(nt))


@pytest.mark.parametrize("dev", [False, True])
def test_argument_errors(pkg, dev):
    bad = [dict(dims=(1, 4, 4)), dict(dims=(4, 4, 1)), dict(dims=(4, 0, 4)), dict(spacing=0.0), dict(spacing=-1.0),
           dict(spacing=float("inf")), dict(spacing=float("nan")), dict(iso=float("nan")), dict(caps=(4, 0)), dict(caps=(0, 4)),
           dict(caps=(-1, 0))]
    for kw in bad:
        assert _call(pkg, dev=dev, **kw) == -1, kw        # R2S_ERR_ARG, before any device work
    lib = pkg._lib.lib()
    nv, nt = ctypes.c_int64(), ctypes.c_int64()
    assert lib.r2s_last_isosurface(None, 1, None, 0, ctypes.byref(nv), ctypes.byref(nt)) == -1
    assert lib.r2s_last_isosurface(None, 0, None, 0, None, ctypes.byref(nt)) == -1
    grid = pkg.Grid(np.zeros(3), np.ones(3), 4, 1)
    with pytest.raises(pkg._lib.R2SError, match="doesn't match"):
        pkg.extract_isosurface(np.zeros(7, np.float32), grid)


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present")
def test_no_cpu_fallback(pkg):
    grid = pkg.Grid(np.zeros(3), np.ones(3), 4, 1)
    with pytest.raises(pkg._lib.R2SError, match="no HIP device|CPU fallback"):
        pkg.extract_isosurface(np.zeros(grid.ngp), grid)
    assert _call(pkg) == -2 and _call(pkg, dev=True) == -2
