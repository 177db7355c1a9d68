"""Host-side parts of the mesh orient (no GPU): the restatement of tests/mesh_orient_ref.py held to the properties the header
promises on every case of tests/mesh_orient_cases.py, plain and scrambled, under both rules; the figures the case descriptions
promise; the refusals of r2s_mesh_orient that come before any device work; the exported symbols and the Julia ccall tuples."""
import ctypes
import os
import re

import numpy as np
import pytest

import mesh_orient_cases as C
import mesh_orient_ref as R
import mesh_shells_ref64 as M
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "rho2sdf_hip.h")
JULIA = os.path.join(ROOT, "rho2sdf.jl_amd", "julia", "Rho2sdfHIP.jl")
INTEGRATION = os.path.join(ROOT, "INTEGRATION.md")
ARG, UNSUPPORTED, NO_DEVICE = -1, -4, -2

_an = {}


def analysis(name, scrambled):
    """the flag-independent part of the restatement, computed once and left unchanged"""
    if (name, scrambled) not in _an:
        _an[(name, scrambled)] = R.analyse(*C.case(name, scrambled))
    return _an[(name, scrambled)]


@pytest.mark.parametrize("name", C.ALL)
def test_restatement_properties(name):
    plain = C.case(name)[1]
    for scrambled in (False, True):
        V, T = C.case(name, scrambled)
        a = analysis(name, scrambled)
        n = len(a["first"])
        # rel and the first triangle: the smallest triangle of every patch, in ascending order, with rel = 0
        assert (np.diff(a["first"]) > 0).all() and (a["rel"][a["first"]] == 0).all()
        assert np.array_equal(a["patch_of_tri"][a["first"]], np.arange(n))
        for p in range(n) if n <= 64 else ():
            assert np.nonzero(a["patch_of_tri"] == p)[0].min() == a["first"][p]
        assert ((a["patch_of_tri"] < 0) == ~a["ok"]).all()
        # no volume decision of these cases is undecidable: |V| is exactly 0 or above its bound
        closed = (a["boundary"] == 0) & (a["nonmanifold"] == 0) & ~a["nonorientable"]
        assert ((a["V"][closed] == 0) | (np.abs(a["V"][closed]) > a["bound"][closed])).all()
        for flags in (0, R.OUTWARD):
            r = R.decide(a, flags)
            assert np.array_equal(r["flip"] == 1, (r["tris"] != T).any(1)) and np.array_equal(np.sort(r["tris"], 1), np.sort(T, 1))
            assert np.array_equal(r["tris"][:, 0], T[:, 0])
            # the output through the shells' restatement: no flipped edge is left unless a patch is non-orientable
            _, _, tot = M.topology(r["tris"])
            assert tot[5] == r["totals"][7]
            if not a["nonorientable"].any():
                assert tot[5] == 0
            if flags & R.OUTWARD:
                assert (r["volume"][closed & (a["V"] != 0)] > 0).all()
                assert np.array_equal((r["counts"][:, 3] & 4) != 0, closed & (a["V"] != 0))
            else:
                assert ((r["counts"][:, 3] & 4) == 0).all()
                assert (2 * r["counts"][:, 2] <= r["counts"][:, 1]).all()          # the majority never flips more than half
            # orienting the result again flips nothing
            again = R.orient(V, r["tris"], flags)
            assert again["totals"][3] == 0 and np.array_equal(again["tris"], r["tris"])
            # the scrambled round trip: where the plain mesh is its own result, the scrambled one comes back to it
            if scrambled and name in ("sphere33", "torus", "tetrahedron", "nested41") and not (name == "nested41" and flags):
                if name != "tetrahedron" or flags:                                  # (4 triangles: the majority may tie)
                    assert np.array_equal(r["tris"], plain)
    if name == "nested41":
        r = R.decide(analysis(name, True), R.OUTWARD)
        neg = R.decide(analysis(name, False), 0)["volume"] < 0
        assert neg.tolist() == [False, True, False]
        assert np.array_equal(r["tris"], C.reverse(plain, neg[analysis(name, False)["patch_of_tri"]]))


def test_restatement_on_the_named_cases():
    """the figures the case descriptions promise"""
    o = lambda name, flags=0, s=False: R.decide(analysis(name, s), flags)   # noqa: E731
    assert o("empty")["totals"].tolist() == [0] * 8 and o("all_collapsed")["totals"].tolist() == [0, 4, 4, 0, 0, 0, 0, 0]
    assert o("one_triangle")["counts"].tolist() == [[0, 1, 0, 0, 3, 0, 0, 0]]
    for name, maj, out in (("tetrahedron", 0, 0), ("tetrahedron_reversed", 0, 4), ("tetrahedron_one_reversed", 1, 1),
                           ("cube_one_reversed", 1, 1)):
        assert o(name)["totals"][3] == maj and o(name, 1)["totals"][3] == out, name
        assert o(name, 1)["totals"][5:7].tolist() == [1, 1] and o(name)["totals"][5:7].tolist() == [1, 0]
    assert o("tetrahedron", 1)["volume"].tolist() == [36000.0] and o("tetrahedron_reversed")["volume"].tolist() == [-36000.0]
    r = o("cube_with_void")
    assert r["totals"][:4].tolist() == [2, 24, 0, 0] and r["volume"].tolist() == [8.0, -1.0]
    r = o("cube_with_void", 1)                       # the caveat: OUTWARD ignores nesting and turns the void into a body
    assert r["flip"].tolist() == [0] * 12 + [1] * 12 and r["volume"].tolist() == [8.0, 1.0] and r["totals"][3] == 12
    r = o("two_same_direction")
    assert r["flip"].tolist() == [0, 1] and r["counts"].tolist() == [[0, 2, 1, 0, 4, 0, 1, 0]]
    for flags in (0, 1):                             # closed, V == 0 exactly: OUTWARD falls through to the tie rule
        r = o("triangle_twice", flags)
        assert r["counts"].tolist() == [[0, 2, 1, 1, 0, 0, 3, 0]] and r["volume"].tolist() == [0.0] and r["flip"].tolist() == [0, 1]
    r = o("three_on_edge")
    assert r["totals"][0] == 3 and r["counts"][:, 4:6].tolist() == [[2, 1]] * 3 and r["totals"][3] == 0
    r = o("fans40")
    assert (r["counts"][:, 1] == np.arange(1, 41)).all() and (r["counts"][:, 3] == 0).all()
    r = o("two_cubes_sharing_edge", 1)
    assert r["totals"][0] == 2 and r["counts"][:, 1:6].tolist() == [[12, 0, 0, 0, 2]] * 2 and r["totals"][5] == 0
    # (the second tetrahedron is the point reflection of the first with the same index pattern: wound inward)
    assert o("two_tets_sharing_vertex", 1)["totals"].tolist() == [2, 8, 0, 4, 0, 2, 2, 0]
    assert o("two_tets_sharing_vertex")["totals"].tolist() == [2, 8, 0, 0, 0, 2, 0, 0]
    r = o("moebius", 1)
    a = analysis("moebius", False)
    assert r["totals"][0] == 1 and r["totals"][4] == 1 and r["totals"][3] == 0 and r["counts"][0, 3] == 2
    assert np.array_equal(r["tris"], C.case("moebius")[1]) and r["totals"][7] == a["flipped_in"][0] >= 1
    r = o("moebius_and_tetrahedron", 1, True)
    assert r["totals"][0] == 2 and r["counts"][:, 3].tolist() == [2, 5] and r["volume"][1] > 0
    r = o("ribbon_alternating")
    assert r["totals"][0] == 1 and r["counts"][0, 1:3].tolist() == [3000, 1500] and r["flip"][:4].tolist() == [0, 1, 0, 1]
    assert o("ribbon_alternating_shuffled")["counts"][0, 1:3].tolist() == [3000, 1500]
    assert o("disjoint")["totals"][0] == 3000
    r = o("torus", 1, True)
    assert r["totals"][0] == 1 and r["counts"][0, 1] == 20000 and r["counts"][0, 3] == 5 and r["totals"][3] > 5000
    for name, s in [(n, s) for n in C.TIE_FREE for s in (False, True)]:
        a = analysis(name, s)
        assert (2 * a["n1"] != a["n_tris"])[~a["nonorientable"]].all(), (name, s)


def test_flip_patches(pkg):
    V, T = C.case("cube_with_void")
    r = R.orient(V, T, R.OUTWARD)
    back = pkg.flip_patches(r["tris"], r["patch_of_tri"], [1])
    assert np.array_equal(back, T) and back is not r["tris"]
    assert np.array_equal(pkg.flip_patches(r["tris"], r["patch_of_tri"], np.array([False, True])), T)
    assert np.array_equal(pkg.flip_patches(T, r["patch_of_tri"], []), T)
    pot = np.array([-1, 0, 0, -1], np.int32)
    t4 = np.arange(12, dtype=np.int32).reshape(4, 3)
    assert pkg.flip_patches(t4, pot, [0]).tolist() == [[0, 1, 2], [3, 5, 4], [6, 8, 7], [9, 10, 11]]
    for bad in ([2], [-1], np.array([True])):
        with pytest.raises(pkg._lib.R2SError):
            pkg.flip_patches(T, r["patch_of_tri"], bad)
    with pytest.raises(pkg._lib.R2SError):
        pkg.flip_patches(T[:5], r["patch_of_tri"], [0])


# ---- the library without a device -----------------------------------------------------------------------------------------

def test_symbols_and_exports(pkg):
    lib = pkg._lib.lib()
    for s in ("r2s_mesh_orient", "r2s_last_mesh_orient", "r2s_mesh_orient_dev"):
        assert hasattr(lib, s) and [x[0] for x in pkg._lib.SYMBOLS].count(s) == 1
    for name in ("MeshOrient", "mesh_orient", "mesh_orient_dev", "flip_patches"):
        assert name in pkg.__all__ and hasattr(pkg, name)
    assert pkg._lib.ORIENT_OUTWARD == 1 and re.search(r"#define R2S_ORIENT_OUTWARD 1\b", open(HEADER).read())


def _call(pkg, V, T, flags=0, nv=None, nt=None, outs=True, tris_out=True, dev=False):
    """-> (rc, outputs untouched?) of one raw call with poisoned outputs (dev: host memory as "device" pointers - every call
    here is refused before anything reads them)"""
    L = pkg._lib
    v, t = np.ascontiguousarray(V, np.float32).reshape(-1, 3), np.ascontiguousarray(T, np.int32).reshape(-1, 3)
    out, flip, pot = np.full((len(t) + 1, 3), -7, np.int32), np.full(len(t) + 1, -7, np.int32), np.full(len(t) + 1, -7, np.int32)
    n, ref, tot = ctypes.c_int64(-7), np.full(3, -7.0), np.full(8, -7, np.int64)
    nv, nt = len(v) if nv is None else nv, len(t) if nt is None else nt
    ip, vp = (lambda x: x.ctypes.data_as(L.c_int32_p)), (lambda x: x.ctypes.data_as(ctypes.c_void_p))
    tail = (ctypes.byref(n) if outs else None, ref.ctypes.data_as(L.c_double_p), tot.ctypes.data_as(L.c_int64_p))
    if dev:
        rc = L.lib().r2s_mesh_orient_dev(vp(v) if len(v) else None, nv, vp(t), nt, flags, vp(out) if tris_out else None, vp(flip), vp(pot),
                                         None, None, 0, *tail, None)
    else:
        rc = L.lib().r2s_mesh_orient(v.ctypes.data_as(L.c_float_p) if len(v) else None, nv, ip(t), nt, flags, -1,
                                     ip(out) if tris_out else None, ip(flip), ip(pot), *tail)
    clean = (out == -7).all() and (flip == -7).all() and (pot == -7).all() and n.value == -7 and (ref == -7.0).all() and (tot == -7).all()
    return rc, bool(clean)


@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
def test_refusals_before_any_device_work(pkg, dev):
    V, T = C.case("cube_with_void")
    for flags in (2, 3, -1, 1 << 20):
        assert _call(pkg, V, T, flags=flags, dev=dev) == (ARG, True), flags
    assert _call(pkg, V, T, nv=-1, dev=dev) == (ARG, True) and _call(pkg, V, T, nt=-1, dev=dev) == (ARG, True)
    assert _call(pkg, V, T, outs=False, dev=dev) == (ARG, True) and _call(pkg, V, T, tris_out=False, dev=dev) == (ARG, True)
    assert _call(pkg, np.zeros((0, 3)), T, nv=8, dev=dev) == (ARG, True)
    assert _call(pkg, V, T, nt=2 ** 30 + 1, dev=dev) == (UNSUPPORTED, True)      # refused before anything is read
    assert "2^30" in pkg._lib.lib().r2s_last_error().decode()
    assert _call(pkg, V, T, nv=2 ** 31, dev=dev) == (UNSUPPORTED, True)
    lib = pkg._lib.lib()
    n = ctypes.c_int64()
    assert lib.r2s_last_mesh_orient(None, None, 4, ctypes.byref(n)) == ARG and lib.r2s_last_mesh_orient(None, None, 0, None) == ARG
    assert lib.r2s_last_mesh_orient(None, None, -1, ctypes.byref(n)) == ARG


def test_host_mesh_check_comes_before_the_device(pkg):
    V, T = C.case("cube_with_void")
    T2, V2, V3 = T.copy(), V.copy(), V.copy()
    T2[7, 1], V2[3, 2], V3[0, 0] = len(V), np.nan, np.inf
    for v, t in ((V, T2), (V, T - 1), (V2, T), (V3, T)):
        assert _call(pkg, v, t) == (ARG, True)
        msg = pkg._lib.lib().r2s_last_error().decode()
        assert msg.startswith("mesh_orient:") and ("not finite" in msg or "outside" in msg)


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present")
def test_no_cpu_fallback(pkg):
    V, T = C.case("tetrahedron")
    assert _call(pkg, V, T) == (NO_DEVICE, True) and _call(pkg, V, T, dev=True) == (NO_DEVICE, True)
    with pytest.raises(pkg._lib.R2SError, match="error -2"):
        pkg.mesh_orient(V, T)


# ---- the Julia binding and the INTEGRATION snippet against the header -------------------------------------------------------

C_TO_JULIA = {"const float *": {"Ptr{Float32}", "Ptr{Cvoid}"}, "const int32_t *": {"Ptr{Int32}", "Ptr{Cvoid}"},
              "int32_t *": {"Ptr{Int32}", "Ptr{Cvoid}"}, "int64_t *": {"Ptr{Int64}", "Ptr{Cvoid}"}, "double *": {"Ptr{Float64}", "Ptr{Cvoid}"},
              "int32_t": {"Int32"}, "int64_t": {"Int64"}, "void *": {"Ptr{Cvoid}"}}


def _c_params(name):
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, open(HEADER).read())
    assert m, f"{name} is not declared in the header"
    out = []
    for p in m.group(1).split(","):
        p = " ".join(p.split())
        arr = p.endswith("]")                        # int64_t totals[8] is int64_t *
        p = re.sub(r"\[\d*\]$", "", p)
        t = re.match(r"(.*?)(\w+)$", p).group(1).strip()
        t = re.sub(r"\s*\*\s*$", " *", t)
        out.append(t + " *" if arr else t)
    return out


def _ccalls(src, name):
    tuples = []
    for m in re.finditer(r"ccall\(\(:%s,\s*(?:LIB\[\]|lib)\),\s*Cint,\s*\(" % name, src):
        i, depth = m.end(), 1
        while depth:
            depth += {"(": 1, ")": -1}.get(src[i], 0)
            i += 1
        tuples.append([x.strip() for x in src[m.end():i - 1].split(",") if x.strip()])
    return tuples


@pytest.mark.parametrize("path", [JULIA, INTEGRATION], ids=["julia", "integration"])
def test_ccall_type_tuples_match_the_header(path):
    src = open(path).read()
    for name in ("r2s_mesh_orient", "r2s_last_mesh_orient", "r2s_mesh_orient_dev"):
        c = _c_params(name)
        calls = _ccalls(src, name)
        if path == INTEGRATION and name != "r2s_mesh_orient":
            continue                                  # (the snippet shows the host call)
        assert calls, f"{name}: no ccall in {os.path.basename(path)}"
        for types in calls:
            assert len(types) == len(c), (name, types, c)
            for jt, ct in zip(types, c):
                assert jt in C_TO_JULIA[ct], (name, jt, ct)
                if name != "r2s_mesh_orient_dev":
                    assert jt != "Ptr{Cvoid}", (name, jt, ct)   # the host variants use typed pointers
    assert "mesh_orient" in src and "OUTWARD" in src.upper()
