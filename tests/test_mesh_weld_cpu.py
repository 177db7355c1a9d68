"""Host-side parts of the mesh weld and the STL import (no GPU): the invariants of the numpy restatement
(tests/mesh_weld_ref.py) on every case, r2s_import_stl on binary and ASCII files, the refusals of r2s_mesh_weld that come before
any device work, and the Julia / INTEGRATION ccall tuples against the header."""
import ctypes
import os
import re

import numpy as np
import pytest

import mesh_weld_cases as C
import mesh_weld_ref as W
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "rho2sdf_hip.h")
JULIA = os.path.join(ROOT, "rho2sdf.jl_amd", "julia", "Rho2sdfHIP.jl")
INTEGRATION = os.path.join(ROOT, "INTEGRATION.md")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- the restatement's own invariants -------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", C.ALL)
def test_restatement_invariants(name):
    V, T, _ = C.case(name)
    Tin = np.arange(len(V), dtype=np.int64).reshape(-1, 3) if T is None else T.astype(np.int64)
    for snap, flags in C.variants(name):
        r = W.weld(V, T, snap, flags)
        nv_out, nt_out = len(r["verts"]), len(r["tris"])
        assert r["totals"][0] == nv_out and r["totals"][1] == nt_out and r["totals"][7] == 0
        # every output vertex is an input vertex, bit for bit, the first of its class, in first-occurrence order
        assert np.array_equal(_bits(r["verts"]), _bits(V[r["rep"]])) and (np.diff(r["rep"]) > 0).all()
        K = W.keys(V, snap)
        same = lambda i, j: tuple(K[i]) == tuple(K[j])   # noqa: E731
        vm, tm = r["vert_map"], r["tri_map"]
        for i in range(len(V)):
            if vm[i] >= 0:
                assert same(i, r["rep"][vm[i]]) and r["rep"][vm[i]] <= i
        assert all(vm[j] == k for k, j in enumerate(r["rep"]))
        # the classes by direct set computation
        classes = {}
        for i in range(len(V)):
            classes.setdefault(tuple(K[i]), []).append(i)
        assert r["totals"][2] == len(V) - len(classes)
        cls = {i: min(m) for m in classes.values() for i in m}
        R = [tuple(cls[i] for i in t) for t in Tin]
        col = [len(set(x)) < 3 for x in R]
        assert r["totals"][3] == sum(col)
        low = lambda x: min(x, (x[1], x[2], x[0]), (x[2], x[0], x[1]))   # noqa: E731  (the smallest of the three rotations)
        firsts, dup = {}, [False] * len(R)
        for t, x in enumerate(R):
            if not col[t]:
                dup[t] = firsts.setdefault(low(x), t) != t
        assert r["totals"][4] == sum(dup)
        opp = {frozenset(x) for x in firsts if low((x[0], x[2], x[1])) in firsts}
        assert r["totals"][5] == len(opp)
        keep = [not (col[t] and flags & 1) and not (dup[t] and flags & 2) for t in range(len(R))]
        assert np.array_equal(tm >= 0, keep) and np.array_equal(tm[tm >= 0], np.arange(nt_out))
        usedc = {c for t, x in enumerate(R) if keep[t] for c in x}
        assert r["totals"][6] == len(classes) - len(usedc)
        assert nv_out == (len(usedc) if flags & 4 else len(classes))
        # survivors: remapped through vert_map, corner order kept
        for t in range(len(R)):
            if keep[t]:
                assert np.array_equal(r["tris"][tm[t]], vm[Tin[t]]) and (vm[Tin[t]] >= 0).all()
        # welding the result again changes nothing (with the same drops)
        r2 = W.weld(r["verts"], r["tris"], snap, flags)
        assert np.array_equal(r2["vert_map"], np.arange(nv_out)) and np.array_equal(r2["tri_map"], np.arange(nt_out))
        assert np.array_equal(_bits(r2["verts"]), _bits(r["verts"])) and np.array_equal(r2["tris"], r["tris"])


def test_restatement_on_the_named_cases():
    """the figures the case descriptions promise"""
    r = W.weld(*C.case("cube_soup")[:2])
    assert r["totals"][0] == 8 and r["totals"][1] == 12 and r["totals"][2] == 28
    r = W.weld(*C.case("all_one_point")[:2], 0.0, 0)
    assert r["totals"].tolist() == [1, 100, 299, 100, 0, 0, 0, 0]
    V, T, _ = C.case("signed_zero")
    r = W.weld(V, T)
    assert r["totals"][2] == 4 and np.array_equal(_bits(r["verts"][:3]), _bits(V[[0, 2, 4]]))
    r = W.weld(*C.case("rotations")[:2], 0.0, 7)
    assert r["totals"][4] == 5 and r["totals"][5] == 2 and r["totals"][1] == 5
    r = W.weld(*C.case("duplicates_after_weld")[:2], 0.0, 7)
    assert r["totals"][4] == 1 and r["totals"][5] == 1 and r["totals"][2] == 6
    V, T, s = C.case("snap_negative")
    q = W.keys(V[:11], s)[:, 0].tolist()
    assert q == [-2, -1, -1, 0, 0, 0, 1, 1, 2, -2, -3]
    V, T, s = C.case("snap_cell_faces")
    vm = W.weld(V, T, s, 0)["vert_map"]
    assert vm[0] != vm[1] and vm[1] == vm[2] and vm[3] != vm[4] and vm[4] == vm[5] and vm[6] != vm[7] and vm[7] == vm[8]
    assert vm[9] != vm[10] and vm[9] == vm[11]
    V, T, s = C.case("denormal_and_huge")
    vm = W.weld(V, T, 0.0, 0)["vert_map"]
    assert vm[0] == vm[2] and len({vm[0], vm[1], vm[3], vm[4]}) == 4 and vm[5] == vm[6] != vm[7]
    with pytest.raises(W.SnapTooFine):
        W.weld(np.ones((3, 3), np.float32), None, 1e-12)
    V, T, _ = C.case("sphere_soup")
    r = W.weld(V, T)
    assert r["totals"][1] == len(V) // 3 and r["totals"][0] < len(V) // 5


# ---- STL import -----------------------------------------------------------------------------------------------------------

ASCII = """SoLiD first part  with a name
  FACET NORMAL 0 0 1
\t\touter   LOOP
      vertex 1e-3 -0.0 1.17549435e-38
      VERTEX\t1 0
 0
      vertex 0 1 0.5
    endloop
  EndFacet
endsolid first part
solid
facet normal nan nan nan outer loop vertex 3 4 5 vertex -6.25 7 8 vertex 9 1e1 11 endloop endfacet
facet normal 0 0 0 outer loop vertex 0.1 0.2 0.3 vertex 16777217 2 3 vertex 4 5 6 endloop endfacet
ENDSOLID"""
ASCII_SOUP = [["1e-3", "-0.0", "1.17549435e-38"], ["1", "0", "0"], ["0", "1", "0.5"], ["3", "4", "5"], ["-6.25", "7", "8"],
              ["9", "1e1", "11"], ["0.1", "0.2", "0.3"], ["16777217", "2", "3"], ["4", "5", "6"]]


def _import_rc(pkg, path):
    m = pkg._lib.R2SStlMesh()
    rc = pkg._lib.lib().r2s_import_stl(str(path).encode(), ctypes.byref(m))
    return rc, m, pkg._lib.lib().r2s_last_error().decode()


def test_import_stl_binary(pkg, tmp_path):
    rng = np.random.default_rng(8)
    v = rng.normal(size=(30, 3)).astype(np.float32)
    v[3] = [-0.0, np.float32(1e-45), np.finfo(np.float32).max]
    t = rng.integers(0, 30, size=(47, 3)).astype(np.int32)
    path = pkg.export_stl(str(tmp_path / "mesh"), v, t)
    soup, tris = pkg.import_stl(path, weld=False)
    assert soup.dtype == np.float32 and tris.dtype == np.int32
    assert np.array_equal(_bits(soup), _bits(v[t.ravel()])) and np.array_equal(tris, np.arange(141).reshape(-1, 3))
    path = pkg.export_stl(str(tmp_path / "none"), v, np.zeros((0, 3), np.int32))
    soup, tris = pkg.import_stl(path, weld=False)
    assert soup.shape == (0, 3) and tris.shape == (0, 3)
    # a binary file whose header begins with "solid" is still binary: the size decides
    data = bytearray(open(pkg.export_stl(str(tmp_path / "s"), v, t), "rb").read())
    data[:5] = b"solid"
    (tmp_path / "solid_header.stl").write_bytes(bytes(data))
    assert np.array_equal(_bits(pkg.import_stl(tmp_path / "solid_header.stl", weld=False)[0]), _bits(v[t.ravel()]))


def test_import_stl_ascii(pkg, tmp_path):
    p = tmp_path / "hand.stl"
    p.write_text(ASCII)
    soup, tris = pkg.import_stl(p, weld=False)
    want = np.array([[np.float32(np.float64(x)) for x in row] for row in ASCII_SOUP], np.float32)   # strtod, rounded once
    assert np.array_equal(_bits(soup), _bits(want)) and np.array_equal(tris, np.arange(9).reshape(3, 3))
    assert _bits(soup[0, 1]) == 0x80000000 and _bits(soup[0, 2]) == 0x00800000 and soup[7, 0] == np.float32(16777216.0)


def test_import_stl_refusals(pkg, tmp_path):
    v = np.eye(3, dtype=np.float32)
    data = open(pkg.export_stl(str(tmp_path / "b"), v, np.array([[0, 1, 2], [2, 1, 0]], np.int32)), "rb").read()
    bad = {"binary_short": data[:-1], "binary_long": data + b"\0", "ascii_short": ASCII[:-1].encode(),
           "ascii_mid_facet": ASCII[:ASCII.index("endloop")].encode(), "empty": b"",
           "two_vertices": b"solid a\nfacet normal 0 0 1\nouter loop\nvertex 0 0 0\nvertex 1 0 0\nendloop\nendfacet\nendsolid a\n",
           "four_vertices": b"solid\nfacet normal 0 0 1 outer loop vertex 0 0 0 vertex 1 0 0 vertex 0 1 0 vertex 1 1 0 endloop endfacet endsolid",
           "not_a_number": b"solid\nfacet normal 0 0 1 outer loop vertex 0 0 0 vertex 1 0 0x vertex 0 1 0 endloop endfacet endsolid",
           "nan": b"solid\nfacet normal 0 0 1 outer loop vertex 0 0 0 vertex 1 nan 0 vertex 0 1 0 endloop endfacet endsolid",
           "overflow": b"solid\nfacet normal 0 0 1 outer loop vertex 0 0 0 vertex 1 1e39 0 vertex 0 1 0 endloop endfacet endsolid"}
    nan_bin = bytearray(data)
    nan_bin[84 + 12:84 + 16] = np.float32(np.nan).tobytes()
    bad["binary_nan"] = bytes(nan_bin)
    for name, content in bad.items():
        p = tmp_path / (name + ".stl")
        p.write_bytes(content)
        rc, m, msg = _import_rc(pkg, p)
        assert rc == -1 and m.n_tris == 0 and not m.verts and name + ".stl" in msg, (name, rc, msg)
        with pytest.raises(pkg._lib.R2SError):
            pkg.import_stl(p, weld=False)
    rc, _, msg = _import_rc(pkg, tmp_path / "two_vertices.stl")
    assert "2 vertices" in msg
    rc, _, msg = _import_rc(pkg, tmp_path / "missing.stl")
    assert rc == -1 and "not found" in msg
    pkg._lib.lib().r2s_free_stl_mesh(None)


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present")
def test_no_cpu_fallback(pkg, tmp_path):
    v = np.eye(3, dtype=np.float32)
    path = pkg.export_stl(str(tmp_path / "t"), v, np.array([[0, 1, 2]], np.int32))
    with pytest.raises(pkg._lib.R2SError, match="error -2"):
        pkg.import_stl(path)                       # weld=True needs the device
    with pytest.raises(pkg._lib.R2SError, match="error -2"):
        pkg.mesh_weld(v)
    assert _weld_rc(pkg, v, None)[0] == -2 and _weld_rc(pkg, v, None, dev=True)[0] == -2


# ---- refusals of r2s_mesh_weld before any device work ---------------------------------------------------------------------

def _weld_rc(pkg, verts, tris, snap=0.0, flags=5, dev=False, n_verts=None, n_tris=None, null_out=False, null_totals=False):
    """-> (rc, outputs untouched?) of one raw call with poisoned outputs"""
    L = pkg._lib
    v = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
    t = None if tris is None else np.ascontiguousarray(tris, np.int32).reshape(-1, 3)
    nv = len(v) if n_verts is None else n_verts
    nt = (len(v) // 3 if t is None else len(t)) if n_tris is None else n_tris
    vo, to = np.full((len(v) + 1, 3), 7.5, np.float32), np.full((len(v) + 8, 3), -7, np.int32)
    vm, tm, tot = np.full(len(v) + 1, -7, np.int32), np.full(len(v) + 8, -7, np.int32), np.full(8, -7, np.int64)
    ip = lambda a: a.ctypes.data_as(L.c_int32_p)   # noqa: E731
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    totp = None if null_totals else tot.ctypes.data_as(L.c_int64_p)
    if dev:   # (host memory as "device" pointers: every call here is refused before anything reads them)
        rc = L.lib().r2s_mesh_weld_dev(vp(v), nv, None if t is None else vp(t), nt, snap, flags, None if null_out else vp(vo), vp(to),
                                       vp(vm), vp(tm), totp, None)
    else:
        rc = L.lib().r2s_mesh_weld(v.ctypes.data_as(L.c_float_p), nv, None if t is None else ip(t), nt, snap, flags, -1,
                                   None if null_out else vo.ctypes.data_as(L.c_float_p), ip(to), ip(vm), ip(tm), totp)
    clean = (vo == 7.5).all() and (to == -7).all() and (vm == -7).all() and (tm == -7).all() and (tot == -7).all()
    return rc, clean


@pytest.mark.parametrize("dev", [False, True])
def test_argument_errors(pkg, dev):
    V = np.arange(18, dtype=np.float32).reshape(6, 3)
    T = np.array([[0, 1, 2], [3, 4, 5]], np.int32)
    bad = [dict(verts=V[:5], tris=None),                      # n_verts % 3 in soup mode
           dict(verts=V, tris=None, n_tris=3),                # a soup has n_verts / 3 triangles
           dict(verts=V, tris=T, snap=-0.5), dict(verts=V, tris=T, snap=float("nan")), dict(verts=V, tris=T, snap=float("inf")),
           dict(verts=V, tris=T, n_verts=-1), dict(verts=V, tris=T, n_tris=-1),
           dict(verts=V, tris=T, flags=8), dict(verts=V, tris=T, null_out=True), dict(verts=V, tris=T, null_totals=True)]
    for kw in bad:
        rc, clean = _weld_rc(pkg, dev=dev, **kw)
        assert rc == -1 and clean, kw
    for kw in (dict(verts=V, tris=T, n_tris=2 ** 30 + 1), dict(verts=V, tris=T, n_verts=2 ** 31)):
        rc, clean = _weld_rc(pkg, dev=dev, **kw)
        assert rc == -4 and clean, kw                         # R2S_ERR_UNSUPPORTED
    assert "2^30" in pkg._lib.lib().r2s_last_error().decode() or "32-bit" in pkg._lib.lib().r2s_last_error().decode()


def test_host_mesh_check_comes_before_the_device(pkg):
    """NaN vertices and out-of-range indices of the host variant are found on the host: R2S_ERR_ARG with or without a GPU"""
    V = np.arange(18, dtype=np.float32).reshape(6, 3)
    T = np.array([[0, 1, 2], [3, 4, 5]], np.int32)
    for v, t in ((np.where(np.arange(18).reshape(6, 3) == 7, np.nan, V).astype(np.float32), T),
                 (np.where(np.arange(18).reshape(6, 3) == 7, np.inf, V).astype(np.float32), None), (V, T + 4), (V, T - 1)):
        rc, clean = _weld_rc(pkg, v, t)
        assert rc == -1 and clean
        msg = pkg._lib.lib().r2s_last_error().decode()
        assert msg.startswith("mesh_weld:") and ("not finite" in msg or "outside" in msg)
    with pytest.raises(pkg._lib.R2SError, match="multiple of 3"):
        pkg.mesh_weld(V[:4])


# ---- the Julia binding and the INTEGRATION snippet against the header -------------------------------------------------------

C_TO_JULIA = {"const char *": {"Cstring"}, "const float *": {"Ptr{Float32}", "Ptr{Cvoid}"}, "float *": {"Ptr{Float32}", "Ptr{Cvoid}"},
              "const int32_t *": {"Ptr{Int32}", "Ptr{Cvoid}"}, "int32_t *": {"Ptr{Int32}", "Ptr{Cvoid}"}, "int64_t *": {"Ptr{Int64}"},
              "double": {"Float64"}, "int32_t": {"Int32"}, "int64_t": {"Int64"}, "void *": {"Ptr{Cvoid}"},
              "r2s_stl_mesh *": {"Ref{R2SStlMesh}"}}
HOST_ONLY = {"Ptr{Float32}", "Ptr{Int32}"}   # what the host variant must use (not an untyped pointer)


def _read(p):
    with open(p) as f:
        return f.read()


def _c_params(name):
    m = re.search(r"\b(?:int|void)\s+%s\s*\(([^)]*)\)\s*;" % name, _read(HEADER))
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


def _ccalls(src, name, ret):
    tuples = []
    for m in re.finditer(r"ccall\(\(:%s,\s*(?:LIB\[\]|lib)\),\s*%s,\s*\(" % (name, ret), src):
        i, depth = m.end(), 1
        while depth:
            depth += {"(": 1, ")": -1}.get(src[i], 0)
            i += 1
        tuples.append([x.strip() for x in src[m.end():i - 1].split(",") if x.strip()])
    return tuples


@pytest.mark.parametrize("path", [JULIA, INTEGRATION], ids=["julia", "integration"])
def test_ccall_type_tuples_match_the_header(path):
    src = _read(path)
    for name, ret in (("r2s_mesh_weld", "Cint"), ("r2s_mesh_weld_dev", "Cint"), ("r2s_import_stl", "Cint"), ("r2s_free_stl_mesh", "Cvoid")):
        c = _c_params(name)
        calls = _ccalls(src, name, ret)
        if path == INTEGRATION and name == "r2s_mesh_weld_dev":
            continue                                  # (the snippet shows the host calls)
        assert calls, f"{name}: no ccall in {os.path.basename(path)}"
        for types in calls:
            assert len(types) == len(c), (name, types, c)
            for jt, ct in zip(types, c):
                assert jt in C_TO_JULIA[ct], (name, jt, ct)
                if name == "r2s_mesh_weld" and ct.endswith("*") and "int64" not in ct:
                    assert jt in HOST_ONLY, (name, jt, ct)
    j = _read(JULIA)
    m = re.search(r"^mutable struct R2SStlMesh\b.*?\n(.*?)^end", j, re.S | re.M)
    fields = [tuple(x.strip() for x in ln.split("#")[0].split("::")) for ln in m.group(1).splitlines() if "::" in ln]
    assert fields == [("n_tris", "Int64"), ("verts", "Ptr{Float32}")]
    for text in (j, src):
        assert "mesh_weld" in text and "import_stl" in text


def test_python_exports(pkg):
    for name in ("MeshWeld", "mesh_weld", "mesh_weld_dev", "import_stl"):
        assert name in pkg.__all__ and hasattr(pkg, name)
    assert ctypes.sizeof(pkg._lib.R2SStlMesh) == 16
    names = [s[0] for s in pkg._lib.SYMBOLS]
    for s in ("r2s_mesh_weld", "r2s_mesh_weld_dev", "r2s_import_stl", "r2s_free_stl_mesh"):
        assert names.count(s) == 1
    assert pkg._lib.lib().r2s_version() == 100
