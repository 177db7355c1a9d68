"""No GPU: the yardstick of tests/test_ray_gpu.py (ray_ref64.raycast_brute, the float64 restatement of the ray query of
include/rho2sdf_hip.h) on known answers, its watertightness, its agreement with exact geometry (mpmath), and the CPU side of
the binding: refusals that need no device, Python argument checks, the declarations in the header, _lib.py and the Julia text."""
import ctypes
import os
import re

import numpy as np
import pytest

import iso_ref
import mesh_dist_ref64 as M
import ray_cases as RC
import ray_ref64 as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG, NO_DEVICE, UNSUPPORTED = -1, -2, -4
INF = np.inf


def _one(V, T, o, d, **kw):
    t, i, s = R.raycast_brute(np.asarray(V, np.float32), np.asarray(T, np.int32), np.array([o], np.float64), np.array([d], np.float64), **kw)
    return float(t[0]), int(i[0]), int(s[0])


TRI = (np.array([[0, 0, 0], [4, 0, 0], [0, 4, 0]], np.float32), np.array([[0, 1, 2]], np.int32))   # normal +z


def test_one_triangle_and_the_side_convention():
    V, T = TRI
    assert _one(V, T, (1, 1, 2), (0, 0, -1)) == (2.0, 0, 1)          # against the normal: enters through the front
    assert _one(V, T, (1, 1, -2), (0, 0, 1)) == (2.0, 0, -1)         # with the normal
    assert _one(V, T, (1, 1, 2), (0, 0, -4)) == (0.5, 0, 1)          # d is not normalised
    assert _one(V, T, (1, 1, 2), (0, 0, 1)) == (INF, -1, 0)          # behind the origin
    assert _one(V, T, (3, 3, 2), (0, 0, -1)) == (INF, -1, 0)         # beside the triangle
    assert _one(V, T, (1.5, 0.5, 1), (-0.5, 0.5, -1)) == (1.0, 0, 1)
    assert _one(V, T[:, [0, 2, 1]], (1, 1, 2), (0, 0, -1)) == (2.0, 0, -1)   # the other winding
    for tgt in ((0, 0, 0), (4, 0, 0), (0, 4, 0), (2, 0, 0), (2, 2, 0), (0, 2, 0)):   # vertices and edges are hit
        assert _one(V, T, (tgt[0], tgt[1], 2), (0, 0, -1)) == (2.0, 0, 1), tgt
    assert _one(V, T, (1, 1, 0), (1, 0, 0)) == (INF, -1, 0)          # in the plane: det == 0
    t, i, s = R.raycast_brute(V, T[:0], np.zeros((3, 3)), np.ones((3, 3)))
    assert np.isposinf(t).all() and (i == -1).all() and (s == 0).all()


def test_unit_square_hit_on_its_diagonal():
    V = np.array([[0, 0, 1], [1, 0, 1], [1, 1, 1], [0, 1, 1]], np.float32)
    T = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    for x in (0.0, 0.25, 0.5, 1.0):
        assert _one(V, T, (x, x, 3), (0, 0, -2)) == (1.0, 0, 1)      # both triangles accept: the smaller index
        assert _one(V, T[::-1], (x, x, -1), (0, 0, 1)) == (2.0, 0, -1)
    assert _one(V, T, (0.25, 0.75, 3), (0, 0, -2)) == (1.0, 1, 1)


def test_axis_aligned_box():
    V, T = M.box_mesh((-1, 0, 2), (3, 2, 2.5))
    o = (0.5, 0.75, 2.25)
    for k, (near, farv) in enumerate(((2.5, 1.5), (1.25, 0.75), (0.25, 0.25))):
        d = np.zeros(3)
        d[k] = 1.0
        t, i, s = _one(V, T, o, d)
        assert (t, s) == (near, -1) and 0 <= i < 12                  # from inside: with the outward normal
        t, i, s = _one(V, T, o, -d)
        assert (t, s) == (farv, -1)
    assert _one(V, T, (-3, 1, 2.25), (1, 0, 0))[::2] == (2.0, 1)
    assert _one(V, T, (-3, 1, 2.25), (1, 0, 0), t_min=2.5)[::2] == (6.0, -1)
    assert _one(V, T, (-3, 1, 2.25), (2, 0.5, 0.125))[::2] == (1.0, 1)
    assert _one(V, T, (-3, 1, 5.0), (1, 0, 0)) == (INF, -1, 0)


def test_window_is_inclusive_at_both_ends():
    V, T = TRI
    o, d = (1, 1, 2), (0, 0, -1)
    assert _one(V, T, o, d, t_min=2.0, t_max=2.0) == (2.0, 0, 1)
    assert _one(V, T, o, d, t_min=0.0, t_max=2.0) == (2.0, 0, 1)
    assert _one(V, T, o, d, t_min=2.0) == (2.0, 0, 1)
    assert _one(V, T, o, d, t_min=2.0 + 2.0 ** -51) == (INF, -1, 0)
    assert _one(V, T, o, d, t_max=2.0 - 2.0 ** -51) == (INF, -1, 0)
    assert _one(V, T, (1, 1, 0), d) == (0.0, 0, 1)                   # t = 0 counts with t_min = 0
    assert _one(V, T, (1, 1, -2), d, t_min=-4.0) == (-2.0, 0, 1)


def test_smallest_index_on_duplicated_triangles():
    V, T = TRI
    far_tri = np.array([[0, 0, -1], [4, 0, -1], [0, 4, -1]], np.float32)
    V2 = np.concatenate([far_tri, V])
    T2 = np.array([[0, 1, 2], [3, 4, 5], [3, 4, 5], [3, 5, 4], [3, 4, 5]], np.int32)
    assert _one(V2, T2, (1, 1, 2), (0, 0, -1)) == (2.0, 1, 1)
    assert _one(V2, T2[[0, 3, 1, 2]], (1, 1, 2), (0, 0, -1)) == (2.0, 1, -1)      # the side is that of the smallest index
    t, i, s = R.raycast_brute(V2, np.repeat(T2[1:2], 5000, axis=0), np.array([[1, 1, 2.0]] * 3), np.array([[0, 0, -1.0]] * 3), budget=4000)
    assert (t == 2.0).all() and (i == 0).all() and (s == 1).all()     # across the chunks of the brute force as well


def test_bad_rays():
    V, T = TRI
    o, d = RC.bad()
    for tris in (T, T[:0]):
        t, i, s = R.raycast_brute(V, tris, o, d)
        assert np.isnan(t).all() and (i == -1).all() and (s == 0).all()


def test_the_restatement_is_watertight():
    """origins within a quarter radius of the centre of a closed sphere surface, rays aimed in float64 at every vertex and
    every edge midpoint: every ray hits, from inside (side -1)"""
    V, T, c, rad = RC.closed_sphere(17)
    dup, missing = iso_ref.unpaired_edges(T.astype(np.int64), len(V))
    assert len(dup) == 0 and len(missing) == 0 and len(T) > 500       # closed and consistently wound
    org = RC.inner_origins(c, rad, 7, 11)
    for name, tg in (("vertices", V.astype(np.float64)), ("edge midpoints", RC.edge_midpoints(V, T))):
        o, d = RC.aimed(org, tg)
        t, i, s = R.raycast_brute(V, T, o, d)
        print(f"RAY watertight {name}: {len(o)} rays at {len(T)} triangles, misses {int(np.isinf(t).sum())}")
        assert np.isfinite(t).all() and (i >= 0).all() and (s == -1).all(), name
        assert (np.abs(t - 1.0) < 1e-9).all(), name                   # d = target - origin: the hit is the target


def _mp_cases():
    """(label, V, T, origins, dirs, (ray, tri) pairs, general) - general cases enter the K ratio, grazing ones do not"""
    rng = np.random.default_rng(21)
    out = []
    V, T, c, rad = RC.closed_sphere(9)
    v = V.astype(np.float64)
    # rays aimed at random interior points of random triangles, from inside and outside, and random pairs
    n = 500
    tri = rng.integers(len(T), size=n)
    w = rng.dirichlet((1.0, 1.0, 1.0), size=n)
    tgt = (v[T[tri]] * w[:, :, None]).sum(axis=1)
    org = np.concatenate([RC.inner_origins(c, rad, n // 2, 5), c + 3.0 * rad * rng.normal(size=(n - n // 2, 3))])
    d = (tgt - org) * rng.uniform(0.25, 4.0, size=(n, 1))
    pairs = [(i, int(tri[i])) for i in range(n)] + [(i, int(rng.integers(len(T)))) for i in range(n)]
    out.append(("sphere 9^3 aimed + random pairs", V, T, org, d, pairs, True))
    # one or two exact zero components, through interior points of triangles
    k = 300
    tri2 = rng.integers(len(T), size=k)
    tgt2 = (v[T[tri2]] * rng.dirichlet((1.0, 1.0, 1.0), size=k)[:, :, None]).sum(axis=1)
    _, d2 = RC.aligned(V, k, 8)
    o2 = tgt2 - d2 * rng.uniform(0.5, 2.0, size=(k, 1))
    out.append(("sphere 9^3 aligned", V, T, o2, d2, [(i, int(tri2[i])) for i in range(k)] +
                [(i, int(rng.integers(len(T)))) for i in range(k)], True))
    # far origins: L is the origin's coordinate
    k = 200
    tri3 = rng.integers(len(T), size=k)
    tgt3 = (v[T[tri3]] * rng.dirichlet((1.0, 1.0, 1.0), size=k)[:, :, None]).sum(axis=1)
    o3, _ = RC.far(V, k, 9)
    out.append(("sphere 9^3 far", V, T, o3, tgt3 - o3, [(i, int(tri3[i])) for i in range(k)], True))
    # grazing: through an interior point of a triangle, nearly in its plane
    m = 400
    tri = rng.integers(len(T), size=m)
    w = rng.dirichlet((2.0, 2.0, 2.0), size=m)
    tgt = (v[T[tri]] * w[:, :, None]).sum(axis=1)
    a, b, cc = v[T[tri, 0]], v[T[tri, 1]], v[T[tri, 2]]
    nrm = np.cross(b - a, cc - a)
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    u = (b - a) * rng.uniform(-1, 1, (m, 1)) + (cc - a) * rng.uniform(-1, 1, (m, 1))
    u /= np.linalg.norm(u, axis=1)[:, None]
    eps = 10.0 ** -rng.uniform(1.0, 11.0, size=(m, 1))    # (flatter ones fall under the edge rule: the projected triangle collapses)
    dg = u + eps * nrm
    og = tgt - dg * rng.uniform(0.5, 3.0, size=(m, 1)) * rad
    out.append(("sphere 9^3 grazing", V, T, og, dg, [(i, int(tri[i])) for i in range(m)], False))
    return out


TAU = 32.0 * R.EPS       # an edge function below TAU R^2 is within the round-off of the sheared products (R = max |vertex - o|)


def test_restatement_against_mpmath():
    """decidable pairs only: an exact edge function within round-off of zero, a t within 1e-9 L of the window's end, or an
    incidence flatter than GRAZING_COS make a pair undecidable; those are counted and capped at 1 % of a case"""
    worst, lost_cos, flattest = 0.0, 0.0, 1.0
    for label, V, T, o, d, pairs, general in _mp_cases():
        v = V.astype(np.float64)
        L = max(float(np.abs(o).max()), float(np.abs(v).max()))
        acc, t, _ = R.pair_table(V, T, o, d)
        undecided, wrong, ratio, nhit = 0, 0, 0.0, 0
        for i, j in pairs:
            r = R.pair_mp(o[i], d[i], v[T[j, 0]], v[T[j, 1]], v[T[j, 2]])
            tl = r["t"] * r["dnorm"] if r["hit"] else None
            edge_close = min(abs(e) for e in r["edges"]) <= TAU and not (min(r["edges"]) < -TAU and max(r["edges"]) > TAU)
            if edge_close or (r["hit"] and abs(tl) <= 1e-9 * L) or (r["hit"] and r["cos"] < R.GRAZING_COS):
                undecided += 1
                continue
            want = bool(r["hit"] and r["t"] >= 0)
            if want:
                flattest = min(flattest, float(r["cos"]))
            if want and not acc[i, j]:
                lost_cos = max(lost_cos, float(r["cos"]))             # lost to the in-box condition (or a rounded edge)
                continue
            if bool(acc[i, j]) != want:
                wrong += 1
                continue
            if want:
                nhit += 1
                if general:
                    ratio = max(ratio, float(abs(t[i, j] - r["t"]) * r["dnorm"] / (R.EPS * L)))
        print(f"RAY mp {label}: {len(pairs)} pairs, {nhit} hits, {undecided} undecidable, {wrong} wrong, ratio {ratio:.3f}")
        assert wrong == 0, label
        assert undecided <= 0.01 * len(pairs), label
        worst = max(worst, ratio)
    print(f"RAY K largest |t_ref - t_mp| |d| / (2^-52 L) = {worst:.3f}; lost to the in-box condition up to |cos| = {lost_cos:.3e}; "
          f"flattest decided hit |cos| = {flattest:.3e}")
    assert worst <= max(2.0 * R.MEASURED_RATIO, 8.0)
    assert lost_cos <= R.GRAZING_COS


def _raycast(pkg, h, o, d, n=None, t_min=0.0, t_max=INF, dev=False, null=()):
    lib = pkg._lib.lib()
    out, tri, side = np.full(len(o), -7.0), np.full(len(o), -7, np.int32), np.full(len(o), -7, np.int8)
    vp = lambda a, k: None if k in null else a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    args = [h, vp(o, "o"), vp(d, "d"), 0, len(o) if n is None else n, t_min, t_max, 0, vp(out, "t"),
            tri.ctypes.data_as(pkg._lib.c_int32_p) if not dev else vp(tri, ""), vp(side, "")]
    rc = lib.r2s_mesh_index_raycast_dev(*args, None) if dev else lib.r2s_mesh_index_raycast(*args)
    assert (out == -7.0).all() and (tri == -7).all() and (side == -7).all()
    return rc


@pytest.mark.parametrize("dev", [False, True])
def test_refusals_need_no_device(pkg, dev):
    o, d = np.zeros((4, 3)), np.ones((4, 3))
    fake = ctypes.c_void_p(8)                                        # never dereferenced: every refusal comes first
    assert _raycast(pkg, None, o, d, dev=dev) == ARG and b"index" in pkg._lib.lib().r2s_last_error()
    assert _raycast(pkg, fake, o, d, n=-1, dev=dev) == ARG
    for k in ("o", "d", "t"):
        assert _raycast(pkg, fake, o, d, dev=dev, null=(k,)) == ARG
    assert _raycast(pkg, fake, o, d, t_min=np.nan, dev=dev) == ARG and _raycast(pkg, fake, o, d, t_max=np.nan, dev=dev) == ARG
    assert _raycast(pkg, fake, o, d, t_min=1.0, t_max=0.5, dev=dev) == ARG and b"t_min" in pkg._lib.lib().r2s_last_error()
    assert _raycast(pkg, fake, o, d, t_min=INF, t_max=-INF, dev=dev) == ARG
    assert _raycast(pkg, fake, o, d, n=2 ** 31, dev=dev) == UNSUPPORTED
    assert _raycast(pkg, fake, o, d, n=0, dev=dev, null=("o", "d", "t")) == 0
    assert _raycast(pkg, fake, o, d, n=0, t_min=np.nan, dev=dev) == ARG


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present")
def test_no_cpu_fallback(pkg):
    V, T = M.box_mesh((0, 0, 0), (1, 1, 1))
    assert _raycast(pkg, ctypes.c_void_p(8), np.zeros((4, 3)), np.ones((4, 3))) == NO_DEVICE
    with pytest.raises(pkg._lib.R2SError, match="no HIP device|CPU fallback"):
        pkg.surface_thickness(V, T, skip=0.125)


def test_python_argument_checks(pkg):
    ix = object.__new__(pkg.MeshIndex)                               # a closed index: every argument check comes first
    ix._h = None
    o, d = np.zeros((4, 3)), np.ones((4, 3))
    E = pkg._lib.R2SError
    with pytest.raises(E, match=r"\(n, 3\)"):
        ix.raycast(o, d[:3])
    with pytest.raises(E, match=r"\(n, 3\)"):
        ix.raycast(o.ravel(), d.ravel())
    with pytest.raises(E, match="dtype"):
        ix.raycast(o, d, dtype=np.float16)
    for kw in (dict(t_min=1.0, t_max=0.0), dict(t_min=np.nan), dict(t_max=np.nan)):
        with pytest.raises(E, match="t_min"):
            ix.raycast(o, d, **kw)
    with pytest.raises(E, match="closed"):
        ix.raycast(o, d)
    V, T = M.box_mesh((0, 0, 0), (1, 1, 1))
    for skip in (-1.0, np.nan, np.inf):
        with pytest.raises(E, match="skip"):
            pkg.surface_thickness(V, T, skip=skip)
    with pytest.raises(TypeError):
        pkg.surface_thickness(V, T)                                  # skip has no default
    with pytest.raises(E, match="normals"):
        pkg.surface_thickness(V, T, np.ones((7, 3)), skip=0.1)
    with pytest.raises(E, match="info"):
        pkg.rho2sdf("t", np.zeros((8, 3)), np.arange(1, 9)[None, :], np.ones(1), thickness=True)


def test_vertex_normals_of_a_box(pkg):
    V, T = M.box_mesh((0, 0, 0), (1, 1, 0.25))
    n = pkg.vertex_normals(V, T)
    assert n.dtype == np.float64 and n.shape == (8, 3)
    assert np.array_equal(np.sign(n), np.sign(V.astype(np.float64) - np.array([0.5, 0.5, 0.125])))   # outward at every corner
    fn = np.cross(V[T[:, 1]].astype(np.float64) - V[T[:, 0]], V[T[:, 2]].astype(np.float64) - V[T[:, 0]])
    want = np.zeros((8, 3))
    for k in range(3):
        for j in range(len(T)):
            want[T[j, k]] += fn[j]
    assert np.array_equal(n, want)


def test_symbols_are_declared_alike(pkg):
    hdr = open(os.path.join(ROOT, "include", "rho2sdf_hip.h")).read()
    jl = open(os.path.join(ROOT, "rho2sdf.jl_amd", "julia", "Rho2sdfHIP.jl")).read()
    ctype = {"const r2s_mesh_index *": "P", "const void *": "P", "void *": "P", "int32_t *": "P", "int8_t *": "P", "int32_t": "i32",
             "int64_t": "i64", "double": "f64"}
    py = {ctypes.c_void_p: "P", pkg._lib.c_int32_p: "P", ctypes.c_int32: "i32", ctypes.c_int64: "i64", ctypes.c_double: "f64"}
    sym = {name: (res, args) for name, res, args in pkg._lib.SYMBOLS}
    sigs = {}
    for name in ("r2s_mesh_index_raycast", "r2s_mesh_index_raycast_dev"):
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", hdr)
        assert m, name
        params = [re.sub(r"\s+", " ", p.strip()) for p in m.group(1).split(",")]
        sigs[name] = [ctype[re.match(r"(.*?)(\w+)$", p).group(1).strip()] for p in params]
        res, args = sym[name]
        assert res is ctypes.c_int and [py[a] for a in args] == sigs[name], name
    assert len(sigs["r2s_mesh_index_raycast"]) == 11 and sigs["r2s_mesh_index_raycast_dev"] == sigs["r2s_mesh_index_raycast"] + ["P"]
    m = re.search(r"ccall\(\(:r2s_mesh_index_raycast, LIB\[\]\), Cint,\s*\(([^)]*)\)", jl)
    assert m and "function mesh_raycast_hip" in jl
    jt = {"Ptr{Cvoid}": "P", "Ptr{Int32}": "P", "Ptr{Int8}": "P", "Int32": "i32", "Int64": "i64", "Float64": "f64"}
    assert [jt[x.strip()] for x in m.group(1).split(",")] == sigs["r2s_mesh_index_raycast"]
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "r2s_mesh_index_raycast" in integ
