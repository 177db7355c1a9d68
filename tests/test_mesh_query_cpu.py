"""No GPU: the CPU side of the mesh index binding (include/rho2sdf_hip.h, r2s_mesh_index_* / r2s_redistance_full) - every
refusal that needs no device returns its code, the compute entry points fail loudly without a device - and the yardstick of
tests/test_mesh_query_gpu.py (mesh_dist_ref64.distance_brute) against the closed-form distance to a box on the point sets of
tests/mesh_query_cases.py, far points included."""
import ctypes
import os
import re

import numpy as np
import pytest

import mesh_dist_ref64 as M
import mesh_query_cases as C

ARG, NO_DEVICE, UNSUPPORTED = -1, -2, -4


def _build(pkg, V, T, nv=None, nt=None, out=True):
    L = pkg._lib
    V, T = np.ascontiguousarray(V, np.float32), np.ascontiguousarray(T, np.int32)
    h = ctypes.c_void_p()
    rc = L.lib().r2s_mesh_index_build(V.ctypes.data_as(L.c_float_p) if V.size else None, len(V) if nv is None else nv,
                                      T.ctypes.data_as(L.c_int32_p) if T.size else None, len(T) if nt is None else nt, -1,
                                      ctypes.byref(h) if out else None)
    return rc, h


def _full(pkg, dims=(4, 4, 4), origin=(0.0, 0.0, 0.0), spacing=0.5, iso=0.0, null=False):
    L = pkg._lib
    f = np.zeros(int(np.prod(dims)), np.float32)
    out = np.full(f.shape, -7.0, np.float32)
    rc = L.lib().r2s_redistance_full(None if null else f.ctypes.data_as(ctypes.c_void_p), 1, (ctypes.c_int64 * 3)(*dims),
                                     (ctypes.c_double * 3)(*origin), spacing, iso, -1, out.ctypes.data_as(ctypes.c_void_p))
    return rc, out


def test_error_codes_match_the_header(pkg):
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rho2sdf_hip.h")).read()
    codes = {k: int(v) for k, v in re.findall(r"#define (R2S_ERR_[A-Z_]+) \((-?\d+)\)", hdr)}
    assert codes["R2S_ERR_ARG"] == ARG and codes["R2S_ERR_NO_DEVICE"] == NO_DEVICE and codes["R2S_ERR_UNSUPPORTED"] == UNSUPPORTED


def test_build_refusals_need_no_device(pkg):
    V, T = M.box_mesh((0, 0, 0), (1, 1, 1))
    T2 = T.copy()
    T2[7, 1] = 8                                                     # == n_verts
    rc, _ = _build(pkg, V, T2)
    assert rc == ARG and b"index" in pkg._lib.lib().r2s_last_error()
    T2[7, 1] = -1
    assert _build(pkg, V, T2)[0] == ARG
    for bad in (np.inf, np.nan):
        V2 = V.copy()
        V2[3, 2] = bad
        assert _build(pkg, V2, T)[0] == ARG
    assert _build(pkg, V, T, nv=-1)[0] == ARG and _build(pkg, V, T, nt=-1)[0] == ARG
    assert _build(pkg, V, T, out=False)[0] == ARG
    assert _build(pkg, np.zeros((0, 3), np.float32), T, nv=8)[0] == ARG        # NULL vertices with a count
    assert _build(pkg, V, T, nt=2 ** 31)[0] == UNSUPPORTED
    assert _build(pkg, V, T, nv=2 ** 31)[0] == UNSUPPORTED


def test_query_refusals_need_no_device(pkg):
    L = pkg._lib
    lib = L.lib()
    p, out = np.zeros((4, 3)), np.full(4, -7.0)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    assert lib.r2s_mesh_index_query(None, vp(p), 0, 4, 0, vp(out), None) == ARG
    assert lib.r2s_mesh_index_query_dev(None, vp(p), 0, 4, 0, vp(out), None, None) == ARG
    info = (ctypes.c_int64 * 4)()
    assert lib.r2s_mesh_index_info(None, info) == ARG
    lib.r2s_mesh_index_destroy(None)                                 # a no-op
    d, o = (ctypes.c_int64 * 3)(4, 4, 4), (ctypes.c_double * 3)(0, 0, 0)
    for fn, extra in ((lib.r2s_mesh_index_lattice, ()), (lib.r2s_mesh_index_lattice_dev, (None,))):
        assert fn(None, d, o, 0.5, 0, vp(out), None, *extra) == ARG
        assert fn(None, (ctypes.c_int64 * 3)(1, 4, 4), o, 0.5, 0, vp(out), None, *extra) == ARG
        assert b"dimension" in lib.r2s_last_error()
        assert fn(None, d, o, 0.0, 0, vp(out), None, *extra) == ARG and b"spacing" in lib.r2s_last_error()
        assert fn(None, d, o, np.inf, 0, vp(out), None, *extra) == ARG and b"spacing" in lib.r2s_last_error()
        assert fn(None, d, (ctypes.c_double * 3)(0, np.nan, 0), 0.5, 0, vp(out), None, *extra) == ARG
        assert b"origin" in lib.r2s_last_error()
    assert (out == -7.0).all()


def test_redistance_full_refusals_need_no_device(pkg):
    bad = [dict(dims=(1, 4, 4)), dict(dims=(4, 4, 1)), dict(spacing=0.0), dict(spacing=-1.0), dict(spacing=np.inf),
           dict(spacing=np.nan), dict(origin=(0.0, np.nan, 0.0)), dict(origin=(np.inf, 0.0, 0.0)), dict(iso=np.nan), dict(null=True)]
    for kw in bad:
        rc, out = _full(pkg, **kw)
        assert rc == ARG and (out == -7.0).all(), kw
    L = pkg._lib
    f = np.zeros(64, np.float32)
    rc = L.lib().r2s_redistance_full_dev(f.ctypes.data_as(ctypes.c_void_p), 1, (ctypes.c_int64 * 3)(4, 4, 1), (ctypes.c_double * 3)(0, 0, 0),
                                         0.5, 0.0, f.ctypes.data_as(ctypes.c_void_p), None)
    assert rc == ARG
    rc = L.lib().r2s_redistance_full(f.ctypes.data_as(ctypes.c_void_p), 1, (ctypes.c_int64 * 3)(2 ** 31, 2, 2),
                                     (ctypes.c_double * 3)(0, 0, 0), 0.5, 0.0, -1, f.ctypes.data_as(ctypes.c_void_p))
    assert rc == UNSUPPORTED


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present")
def test_no_cpu_fallback(pkg):
    V, T = M.box_mesh((0, 0, 0), (1, 1, 1))
    rc, h = _build(pkg, V, T)
    assert rc == NO_DEVICE and not h.value
    rc, out = _full(pkg)
    assert rc == NO_DEVICE and (out == -7.0).all()
    with pytest.raises(pkg._lib.R2SError, match="no HIP device|CPU fallback"):
        pkg.MeshIndex(V, T)
    with pytest.raises(pkg._lib.R2SError, match="no HIP device|CPU fallback"):
        pkg.redistance_full(np.zeros((4, 4, 4), np.float32), pkg.Grid([0, 0, 0], [1, 1, 1], 3, 0))
    with pytest.raises(pkg._lib.R2SError, match="no HIP device|CPU fallback"):
        pkg.surface_deviation(V, T, V + np.float32(0.25), T)


def test_python_argument_checks(pkg):
    with pytest.raises(pkg._lib.R2SError, match="info"):
        pkg.rho2sdf("t", np.zeros((8, 3)), np.arange(1, 9)[None, :], np.ones(1), signed_distance=True)
    with pytest.raises(pkg._lib.R2SError, match="info"):
        pkg.rho2sdf("t", np.zeros((8, 3)), np.arange(1, 9)[None, :], np.ones(1), deviation=True)


def test_brute_force_against_closed_form_on_the_query_sets():
    """the yardstick of the GPU tests on their point sets: inside the box, at 10^3 times its size, on the vertices"""
    lo, hi = (-0.75, 0.5, 1.0), (1.25, 2.0, 1.5)
    V, T = M.box_mesh(lo, hi)
    sets = {"box": C.box_points(np.array(lo) - 1.0, np.array(hi) + 1.0, 4096, 1), "far": C.far_points(lo, hi, 512, 2),
            "vertices": V.astype(np.float64)}
    for name, P in sets.items():
        d, idx = M.distance_brute(V, T, P)
        want = M.box_distance(P, lo, hi)
        L = max(float(np.abs(P).max()), float(np.abs(V).max()))
        frac = np.abs(d - want) / M.bound(want, L, np.float64)
        print(f"MESHQ yardstick {name}: {len(P)} points, largest fraction of the bound {frac.max():.3f} (L = {L:.3f})")
        assert frac.max() <= 1.0, name
        assert ((idx >= 0) & (idx < 12)).all()
    assert (M.distance_brute(V, T, sets["vertices"])[0] == 0.0).all()
    d, idx = M.distance_brute(V, T[:0], sets["box"][:5])
    assert np.isinf(d).all() and (idx == -1).all()
