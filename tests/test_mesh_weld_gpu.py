"""The mesh weld on the GPU (include/rho2sdf_hip.h, r2s_mesh_weld) against the numpy restatement tests/mesh_weld_ref.py.
Everything is integer or copy work, so everything is compared for equality: verts_out bit for bit, tris_out, both maps and the
totals; the host and the _dev variant against each other; two calls in a row.  Then the STL round trip through the shells, a
field with exact-iso lattice points, the snap range refusal and the refusals that need the device check kernel."""
import ctypes

import numpy as np
import pytest

import iso_ref as R
import mesh_shells_cases as S
import mesh_weld_cases as C
import mesh_weld_ref as W

pytestmark = pytest.mark.gpu

_refs = {}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _ref(name, snap, flags):
    if (name, snap, flags) not in _refs:
        V, T, _ = C.case(name)
        _refs[name, snap, flags] = W.weld(V, T, snap, flags)
    return _refs[name, snap, flags]


def _kw(flags):
    return dict(drop_collapsed=bool(flags & 1), drop_duplicates=bool(flags & 2), drop_unused=bool(flags & 4))


def _host(pkg, V, T, snap, flags):
    w = pkg.mesh_weld(V, T, snap=snap, device=0, **_kw(flags))
    return w.verts, w.tris, w.vert_map, w.tri_map, w.totals


def _dev(pkg, V, T, snap, flags):
    import torch
    dV = torch.from_numpy(np.ascontiguousarray(V)).to("cuda:0")
    dT = None if T is None else torch.from_numpy(np.ascontiguousarray(T)).to("cuda:0")
    w = pkg.mesh_weld_dev(dV, dT, snap=snap, **_kw(flags))
    return tuple(x.cpu().numpy() for x in (w.verts, w.tris, w.vert_map, w.tri_map)) + (w.totals,)


def _equal(label, got, want):
    names = ("verts", "tris", "vert_map", "tri_map", "totals")
    for n, g, w in zip(names, got, want):
        assert g.shape == w.shape and g.dtype == w.dtype, (label, n, g.shape, w.shape, g.dtype, w.dtype)
        same = np.array_equal(_bits(g), _bits(w)) if n == "verts" else np.array_equal(g, w)
        assert same, f"{label}: {n} differs" + (f" ({g.tolist()} != {w.tolist()})" if n == "totals" else "")


@pytest.mark.parametrize("name", C.ALL)
def test_cases_equal_the_restatement(pkg, name):
    V, T, _ = C.case(name)
    for snap, flags in C.variants(name):
        r = _ref(name, snap, flags)
        want = (r["verts"], r["tris"], r["vert_map"], r["tri_map"], r["totals"])
        label = f"{name} snap={snap} flags={flags}"
        h = _host(pkg, V, T, snap, flags)
        d = _dev(pkg, V, T, snap, flags)
        print(f"WELD {label}: totals {h[4].tolist()} (restatement {r['totals'].tolist()})")
        _equal(label + " host", h, want)
        _equal(label + " dev", d, want)
        _equal(label + " host, second call", _host(pkg, V, T, snap, flags), h)
        _equal(label + " dev, second call", _dev(pkg, V, T, snap, flags), d)


def test_indexed_input_equals_its_soup(pkg):
    """an indexed mesh and its soup weld to the same mesh when every vertex is used (first-occurrence order aside)"""
    V, T = S.case("sphere33")
    a = pkg.mesh_weld(V, T, device=0)
    b = pkg.mesh_weld(V[T.ravel()], None, device=0)
    assert a.n_merged == 0 and a.n_tris == b.n_tris == len(T) and a.n_verts == b.n_verts == len(V)
    assert np.array_equal(_bits(a.verts[a.tris]), _bits(b.verts[b.tris]))


def _first_occurrence(V, T):
    """the mesh renumbered so that its vertices come in the order in which the triangles first use them"""
    flat = T.ravel()
    _, first = np.unique(flat, return_index=True)
    order = flat[np.sort(first)]
    new = np.full(len(V), -1, np.int32)
    new[order] = np.arange(len(order), dtype=np.int32)
    return V[order], new[T]


def test_stl_round_trip_through_the_shells(pkg, tmp_path):
    from test_mesh_query_gpu import _surface
    # chosen on the CPU: a field whose restated vertices are all distinct points, so the weld must give the mesh back
    for name in ("gyroid17", "sphere33", "nested41"):
        n, f = S.fields()[name]
        Vr, _ = R.vertices(f, (n, n, n), S.ORIGIN, S.SPACING, 0.0)
        if len(np.unique(W.keys(Vr, 0.0), axis=0)) == len(Vr):
            break
    assert len(np.unique(W.keys(Vr, 0.0), axis=0)) == len(Vr), "no fixture field without coincident vertices"
    V, T = _surface(pkg, f, (n, n, n), S.ORIGIN, S.SPACING)
    assert np.array_equal(_bits(V), _bits(Vr)) and len(np.unique(T)) == len(V)
    path = pkg.export_stl(str(tmp_path / name), V, T)
    Vw, Tw = pkg.import_stl(path, weld=True, device=0)
    V1, T1 = _first_occurrence(V, T)
    assert np.array_equal(_bits(Vw), _bits(V1)) and np.array_equal(Tw, T1)
    a, b = pkg.mesh_shells(Vw, Tw, device=0), pkg.mesh_shells(V1, T1, device=0)
    orig = pkg.mesh_shells(V, T, device=0)
    assert np.array_equal(a.counts, b.counts) and np.array_equal(a.totals, b.totals) and np.array_equal(a.shell_of_tri, b.shell_of_tri)
    assert np.array_equal(a.closed, orig.closed) and a.n_shells == orig.n_shells
    assert np.array_equal(a.counts, orig.counts) and np.array_equal(a.totals, orig.totals)
    if name == "sphere33":
        assert a.n_shells == 1 and a.closed.all()
    print(f"WELD round trip {name}: {len(V)} vertices, {len(T)} triangles, {a.n_shells} shells, closed {a.closed.tolist()[:4]}")
    Vs, Ts = pkg.import_stl(path, weld=False)
    soup = pkg.mesh_shells(Vs, Ts, device=0)
    assert soup.n_shells == len(T) and (soup.n_boundary == 3).all()


def test_exact_iso_lattice_points(pkg):
    """Integer-valued fields with lattice points exactly on the iso level.  f = x - 5 (the plane of tests/test_redistance_gpu.py):
    its vertices sit on lattice points, but only x edges cross, one vertex each - measured on the GPU: 63 vertices, 96 triangles,
    nothing coincides, totals[2] = totals[3] = 0 - so it is held to the restatement only.  f = 2 - (|x-5| + |y-4| + |z-3|) (an
    octahedron with integer values): a lattice point with f = 0 is interior and has several exterior neighbours, every such edge
    puts a vertex ON that point (t = 0), and the triangles between them have zero area: the extraction leaves coincident
    vertices, the weld merges them (totals[2] > 0) and the triangles between them collapse (totals[3] > 0)."""
    from test_mesh_query_gpu import _surface
    dims, origin, h = (12, 9, 7), (0.5, -0.25, 2.0), 0.5
    k, j, i = np.meshgrid(np.arange(7.0), np.arange(9.0), np.arange(12.0), indexing="ij")
    fields = {"plane x = 5": i - 5.0, "octahedron": 2.0 - (np.abs(i - 5.0) + np.abs(j - 4.0) + np.abs(k - 3.0))}
    for name, f in fields.items():
        V, T = _surface(pkg, f.ravel(), dims, origin, h)
        for flags in (1 | 4, 7, 0):
            r = W.weld(V, T, 0.0, flags)
            got = _host(pkg, V, T, 0.0, flags)
            _equal(f"{name} flags={flags}", got, (r["verts"], r["tris"], r["vert_map"], r["tri_map"], r["totals"]))
            _equal(f"{name} flags={flags} dev", _dev(pkg, V, T, 0.0, flags), got)
        w = pkg.mesh_weld(V, T, device=0)
        print(f"WELD {name}: {len(V)} vertices, {len(T)} triangles, totals {w.totals.tolist()}")
        assert w.n_tris == len(T) - w.totals[3] and w.n_verts + w.totals[2] + w.totals[6] == len(V)
    assert w.totals[2] > 0 and w.totals[3] > 0                     # (the octahedron)
    sh = pkg.mesh_shells(w.verts, w.tris, device=0)
    print(f"WELD octahedron welded: shells totals {sh.totals.tolist()}")


def _raw(pkg, V, T, snap, dev, flags=5):
    """one raw call with poisoned outputs -> (rc, message, outputs untouched?)"""
    import torch
    L = pkg._lib
    nv, nt = len(V), (len(V) // 3 if T is None else len(T))
    tot = np.full(8, -7, np.int64)
    if dev:
        dV = torch.from_numpy(np.ascontiguousarray(V)).to("cuda:0")
        dT = None if T is None else torch.from_numpy(np.ascontiguousarray(T)).to("cuda:0")
        vo = torch.full((nv, 3), 7.5, dtype=torch.float32, device="cuda:0")
        to, vm, tm = (torch.full(s, -7, dtype=torch.int32, device="cuda:0") for s in ((nt, 3), (nv,), (nt,)))
        p = lambda x: ctypes.c_void_p(x.data_ptr())   # noqa: E731
        rc = L.lib().r2s_mesh_weld_dev(p(dV), nv, None if dT is None else p(dT), nt, snap, flags, p(vo), p(to), p(vm), p(tm),
                                       tot.ctypes.data_as(L.c_int64_p), None)
        torch.cuda.synchronize()
        vo, to, vm, tm = (x.cpu().numpy() for x in (vo, to, vm, tm))
    else:
        vo = np.full((nv, 3), 7.5, np.float32)
        to, vm, tm = (np.full(s, -7, np.int32) for s in ((nt, 3), (nv,), (nt,)))
        ip = lambda a: a.ctypes.data_as(L.c_int32_p)   # noqa: E731
        rc = L.lib().r2s_mesh_weld(V.ctypes.data_as(L.c_float_p), nv, None if T is None else ip(T), nt, snap, flags, 0,
                                   vo.ctypes.data_as(L.c_float_p), ip(to), ip(vm), ip(tm), tot.ctypes.data_as(L.c_int64_p))
    clean = (vo == 7.5).all() and (to == -7).all() and (vm == -7).all() and (tm == -7).all() and (tot == -7).all()
    return rc, L.lib().r2s_last_error().decode(), clean


@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
def test_refusals_that_need_the_device(pkg, dev):
    V = np.ascontiguousarray(np.random.default_rng(2).random((30, 3)), np.float32)   # unit-size coordinates
    T = np.arange(30, dtype=np.int32).reshape(10, 3)
    rc, msg, clean = _raw(pkg, V, None, 1e-12, dev)
    assert rc == -1 and clean and "snap" in msg and "too fine" in msg, (rc, msg)
    rc, msg, clean = _raw(pkg, V, T, 1e-12, dev)
    assert rc == -1 and clean and "too fine" in msg
    rc, msg, clean = _raw(pkg, V * np.float32(3e38), None, 1e-280, dev)              # the quotient is not finite
    assert rc == -1 and clean and "too fine" in msg
    Vn = V.copy()
    Vn[17, 1] = np.nan
    for v, t in ((Vn, None), (Vn, T), (V, T + 21), (V, T - 1)):
        rc, msg, clean = _raw(pkg, v, None if t is None else np.ascontiguousarray(t), 0.0, dev)
        assert rc == -1 and clean and msg.startswith("mesh_weld:") and ("finite" in msg or "outside" in msg), (rc, msg)
    rc, msg, clean = _raw(pkg, V, T, 2.0 ** -20, dev)                                 # (the largest cell index is 2^20: fine)
    assert rc == 0 and not clean
    pkg._lib.lib().r2s_release_cache()                                               # frees the weld's work buffers too
    rc, msg, clean = _raw(pkg, V, T, 0.0, dev)
    assert rc == 0
