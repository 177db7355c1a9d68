"""The point evaluator's yardstick and host logic, without a GPU: the float64 restatement field_ref64 tied to the pinned
lattice restatement rbf_ref64 and to its own finite differences, the argument errors of the r2s_rbf_field entry points,
and the Julia binding's type tuples against the header."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import field_ref64 as F
import rbf_ref64 as R64
from conftest import ROOT, load_fixture

HEADER = os.path.join(ROOT, "include", "rho2sdf_hip.h")
JULIA = os.path.join(ROOT, "rho2sdf.jl_amd", "julia", "Rho2sdfHIP.jl")
LO, H = np.array([0.013, -0.2, 0.07]), 0.1037   # the non-dyadic lattice of the RBF tests


def _grid(pkg, dims):
    dims = np.array(dims)
    g = pkg.Grid(LO, LO + H * (dims - 1.0), int(dims.max()) - 1, 0)
    assert g.dims == tuple(int(d) for d in dims)
    return g


def _field(g, w, thr, th=0.0):
    return F.Field(w, np.array(g.c.aabb_min[:]), np.array(g.c.aabb_max[:]), [int(n) for n in g.c.N], float(g.c.cell_size), thr, th)


def _lattice_points(axes):
    tx, ty, tz = axes
    Z, Y, X = np.meshgrid(tz, ty, tx, indexing="ij")
    return np.stack([X.ravel(), Y.ravel(), Z.ravel()], axis=1).astype(np.float32)


@pytest.mark.parametrize("smooth", [1, 2])
@pytest.mark.parametrize("thr", [1e-2, 1e-3])
def test_restatement_equals_the_lattice_restatement(pkg, thr, smooth):
    """on lattice points the point restatement is rbf_ref64.evaluate: same taps, same Float64 value up to the order of
    the Float64 sum"""
    g = _grid(pkg, (9, 8, 10))
    rng = np.random.default_rng(5)
    w = rng.standard_normal((10, 8, 9)).astype(np.float32)
    amin, amax, N = np.array(g.c.aabb_min[:]), np.array(g.c.aabb_max[:]), [int(n) for n in g.c.N]
    caxes, taxes = R64.coarse_axes(amin, amax, N), R64.fine_axes(amin, amax, N, smooth)
    e = R64.evaluate(w, caxes, taxes, smooth, float(g.c.cell_size), thr)
    assert (e["tie_d2"] < 0).all() and int(e["m"].max()) <= F.KNN                       # no cap at these thresholds
    r = _field(g, w, thr).evaluate(_lattice_points(taxes))
    assert np.array_equal(r["m"], e["m"].ravel()) and not r["capped"].any()
    assert (r["slack"] == 0).all()                                                     # (rbf_ref64 asserted the same)
    assert np.abs(r["val"] - e["val"].ravel()).max() <= 1e-13 * max(1.0, float(e["S"].max()))
    assert np.abs(r["S"] - e["S"].ravel()).max() <= 1e-13 * float(e["S"].max())


def test_restatement_gradient_is_the_derivative_of_its_value(pkg):
    """with the cutoff switched off the function is smooth: central differences of the value in float64"""
    g = _grid(pkg, (9, 8, 10))
    rng = np.random.default_rng(6)
    w = rng.standard_normal((10, 8, 9)).astype(np.float32)
    fld = _field(g, w, 1e-3, th=0.25)
    amin, amax = np.array(g.c.aabb_min[:]), np.array(g.c.aabb_max[:])
    p = (amin + 2.5 * H + rng.random((200, 3)) * (amax - amin - 5.0 * H)).astype(np.float32)
    # Float32 points: a step of 2^-7 cell sizes around a point rounded to a multiple of 2^-12 moves within exact numbers
    q = np.round(p.astype(np.float64) * 4096.0) / 4096.0
    step = 2.0 ** -10
    r = fld.evaluate(q.astype(np.float32), cutoff=False)
    for a in range(3):
        e = np.zeros(3)
        e[a] = step
        hi, lo = (q + e).astype(np.float32), (q - e).astype(np.float32)
        assert np.array_equal(hi.astype(np.float64), q + e) and np.array_equal(lo.astype(np.float64), q - e)
        # the box of a point follows its cell: keep the three evaluations on one node set by staying inside the cell
        fd = (fld.evaluate(hi, cutoff=False)["val"] - fld.evaluate(lo, cutoff=False)["val"]) / (2.0 * step)
        scale = np.abs(r["grad"]).max()
        # cutoff off: a node entering / leaving the box adds at most exp(-(B)^2) ~ 1e-7 relative; the step's own error
        # is step^2 f''' / 6
        assert np.abs(fd - r["grad"][:, a]).max() <= 2e-4 * scale


def test_restatement_cap_and_special_points(pkg):
    g = _grid(pkg, (12, 12, 12))
    rng = np.random.default_rng(7)
    w = rng.standard_normal((12, 12, 12)).astype(np.float32)
    fld = _field(g, w, 1e-5, th=-0.5)
    amin, amax = np.array(g.c.aabb_min[:]), np.array(g.c.aabb_max[:])
    p = (amin + 4.0 * H + rng.random((50, 3)) * (amax - amin - 8.0 * H)).astype(np.float32)
    p = np.vstack([p, [[np.nan, 0, 0]], [[0, np.inf, 0]], [amax + 50.0 * H]]).astype(np.float32)
    r = fld.evaluate(p)
    assert r["capped"][:50].all() and (r["m"][:50] == F.KNN).all()                    # 155-174 nodes in the support
    assert np.isnan(r["val"][50:52]).all() and np.isnan(r["grad"][50:52]).all() and (r["m"][50:52] == 0).all()
    assert r["val"][52] == -0.5 and (r["grad"][52] == 0).all() and r["m"][52] == 0
    out = fld.project(p, 4, 1e-6)
    assert (out["status"][50:52] == 3).all() and out["status"][52] == 2


def test_argument_errors_before_any_device_work(pkg):
    lib, L = pkg._lib.lib(), pkg._lib
    g = _grid(pkg, (5, 5, 5))
    w = np.zeros(125, np.float32)
    wp = w.ctypes.data_as(L.c_float_p)
    h = ctypes.c_void_p()
    ARG = -1
    for thr in (0.0, 1.0, 1e-11, float("nan"), -1.0):
        assert lib.r2s_rbf_field_from_weights(wp, ctypes.byref(g.c), thr, 0.0, -1, ctypes.byref(h)) == ARG
        assert lib.r2s_rbf_field_fit(w.astype(np.float64).ctypes.data_as(L.c_double_p), ctypes.byref(g.c), 1, thr, 1.0, -1,
                                     ctypes.byref(h), None, None) == ARG
    assert lib.r2s_rbf_field_from_weights(None, ctypes.byref(g.c), 1e-3, 0.0, -1, ctypes.byref(h)) == ARG
    assert lib.r2s_rbf_field_from_weights(wp, None, 1e-3, 0.0, -1, ctypes.byref(h)) == ARG
    assert lib.r2s_rbf_field_from_weights(wp, ctypes.byref(g.c), 1e-3, 0.0, -1, None) == ARG
    assert lib.r2s_rbf_field_fit(None, ctypes.byref(g.c), 1, 1e-3, 1.0, -1, ctypes.byref(h), None, None) == ARG
    p = np.zeros((4, 3), np.float32)
    pp = p.ctypes.data_as(L.c_float_p)
    assert lib.r2s_rbf_field_eval(None, pp, 4, pp, None, None) == ARG
    assert lib.r2s_rbf_field_eval_dev(None, None, 0, None, None, None, None) == ARG
    assert lib.r2s_rbf_field_normals(None, pp, 4, pp) == ARG
    assert lib.r2s_rbf_field_normals_dev(None, None, 4, None, None) == ARG
    assert lib.r2s_rbf_field_project(None, pp, 4, 8, 1e-4, None, None, None) == ARG
    assert lib.r2s_rbf_field_project_dev(None, None, 4, 8, 1e-4, None, None, None, None) == ARG
    assert lib.r2s_rbf_field_weights(None, None, None) == ARG
    lib.r2s_rbf_field_destroy(None)                                                    # a no-op
    assert h.value is None
    with pytest.raises(L.R2SError, match="weights length"):
        pkg.RbfField(np.zeros(7, np.float32), g)
    with pytest.raises(L.R2SError, match="sdf length"):
        pkg.fit_rbf_field(np.zeros(7), g, True, 1.0)


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present")
def test_no_device_no_field(pkg):
    g = _grid(pkg, (5, 5, 5))
    with pytest.raises(pkg._lib.R2SError, match="no HIP device|CPU fallback"):
        pkg.fit_rbf_field(np.ones(125), g, True, 1.0)
    with pytest.raises(pkg._lib.R2SError, match="no HIP device|CPU fallback"):
        pkg.RbfField(np.ones(125, np.float32), g)
    lib, L = pkg._lib.lib(), pkg._lib
    h = ctypes.c_void_p()
    w = np.ones(125)
    assert lib.r2s_rbf_field_fit(w.ctypes.data_as(L.c_double_p), ctypes.byref(g.c), 1, 1e-3, 1.0, -1, ctypes.byref(h), None,
                                 None) == -2                                            # R2S_ERR_NO_DEVICE


# ---- the Julia binding against the header (no Julia toolchain in the build image: parsed from the source) ------------

C_TO_JULIA = {
    "const double *": {"Ptr{Float64}"},
    "const float *": {"Ptr{Float32}"},
    "float *": {"Ptr{Float32}", "Ref{Float32}"},
    "int32_t *": {"Ptr{Int32}", "Ref{Int32}"},
    "const r2s_grid *": {"Ref{R2SGrid}"},
    "const r2s_rbf_field *": {"Ptr{Cvoid}"},
    "r2s_rbf_field *": {"Ptr{Cvoid}"},
    "r2s_rbf_field **": {"Ref{Ptr{Cvoid}}"},
    "double": {"Float64"},
    "float": {"Float32"},
    "int32_t": {"Int32"},
    "int64_t": {"Int64"},
    "void *": {"Ptr{Cvoid}"},
}
FIELD_SYMBOLS = ("r2s_rbf_field_fit", "r2s_rbf_field_from_weights", "r2s_rbf_field_weights", "r2s_rbf_field_eval",
                 "r2s_rbf_field_normals", "r2s_rbf_field_project")


def _c_params(name, ret="int"):
    m = re.search(r"\b%s\s+%s\s*\(([^)]*)\)\s*;" % (ret, name), open(HEADER).read())
    assert m, f"{name} is not declared in the header"
    out = []
    for p in m.group(1).split(","):
        p = " ".join(p.split())
        t = re.match(r"(.*?)(\w+)$", p).group(1).strip()
        out.append(re.sub(r"\s*(\*+)\s*$", r" \1", t))
    return out


def _julia_ccalls(name, ret="Cint"):
    src = open(JULIA).read()
    tuples = []
    for m in re.finditer(r"ccall\(\(:%s,\s*LIB\[\]\),\s*%s,\s*\(" % (name, ret), src):
        i, depth = m.end(), 1
        while depth:
            depth += {"(": 1, ")": -1}.get(src[i], 0)
            i += 1
        parts, d, cur = [], 0, ""
        for ch in src[m.end():i - 1]:
            d += {"{": 1, "(": 1, "}": -1, ")": -1}.get(ch, 0)
            if ch == "," and d == 0:
                parts.append(cur.strip())
                cur = ""
            else:
                cur += ch
        if cur.strip():
            parts.append(cur.strip())
        tuples.append(parts)
    return tuples


def test_julia_field_ccalls_match_the_header():
    for name in FIELD_SYMBOLS:
        c, calls = _c_params(name), _julia_ccalls(name)
        assert calls, f"{name}: no ccall in the Julia binding"
        for types in calls:
            assert len(types) == len(c), (name, types, c)
            for jt, ct in zip(types, c):
                assert jt in C_TO_JULIA[ct], (name, jt, ct)
    assert _c_params("r2s_rbf_field_destroy", "void") == ["r2s_rbf_field *"]
    assert _julia_ccalls("r2s_rbf_field_destroy", "Cvoid") == [["Ptr{Cvoid}"]]
    # the _dev variants: the host variant's parameters (device pointers) + the stream
    for name in ("r2s_rbf_field_eval", "r2s_rbf_field_normals", "r2s_rbf_field_project"):
        assert _c_params(name + "_dev") == _c_params(name) + ["void *"]
    # the ctypes mirror has one entry per parameter too
    from importlib.util import module_from_spec, spec_from_file_location
    spec = spec_from_file_location("_r2s_lib_only", os.path.join(ROOT, "rho2sdf.jl_amd", "_lib.py"))
    L = module_from_spec(spec)
    spec.loader.exec_module(L)
    table = {n: a for n, _, a in L.SYMBOLS}
    for name in FIELD_SYMBOLS + tuple(n + "_dev" for n in FIELD_SYMBOLS[3:]):
        assert len(table[name]) == len(_c_params(name)), name
